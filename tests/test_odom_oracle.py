"""The numpy restatement of the base estimate (tests/odom_ref.py) on the CPU: the vectorised law against the foot-by-foot loop, every branch of
branch_case, the words the law must leave alone, what single precision costs, and the walking loop whose controller links see only the estimate --
the measured figures that include/wbc_hip.h quotes."""
import numpy as np
import pytest

from tests import odom_ref as R
from tests.util import relerr


@pytest.fixture(scope="module")
def total_mass(flat_model):
    return float(np.sum(flat_model["mass"]))


@pytest.mark.parametrize("planes", [True, False])
@pytest.mark.parametrize("n", R.PARITY_SIZES)
def test_vectorised_law_equals_the_loop_and_every_branch_is_taken(flat_model, total_mass, n, planes):
    P = R.params()
    c = R.branch_case(flat_model, total_mass, n, rank=n, planes=planes)
    a, b = R.run(P, flat_model, c), R.run(P, flat_model, c, fn=R.estimate_loop)
    for key in ("base", "anchor", "odo", "q_est", "v_est"):
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert np.all(np.isfinite(a["base"]))                      # the NaN of rows 0-2 and of the unanchored feet reached nothing
    if n >= 16:
        for lo in range(0, n - 15, 16):                        # in every 16 states
            part = {key: a[key][lo:lo + 16] for key in ("S", "A", "had")}
            assert R.branches_taken(part) == R.ALL_BRANCHES, lo
        # both reasons for distrust occur
        S = a["S"]
        assert np.any(~S & R._bits(c["contact"])) and np.any(~S & R._bits(c["mask"]))
    assert np.all(c["odo"] & R.JUNK_BITS == R.JUNK_BITS)        # the words carry bits outside 0-3


@pytest.mark.parametrize("planes", [True, False])
def test_untouched_words_and_the_odo_word(flat_model, total_mass, planes):
    n = 33
    P = R.params()
    c = R.branch_case(flat_model, total_mass, n, rank=n, planes=planes)
    e = R.run(P, flat_model, c)
    w = R.written(e)
    assert w.any() and (~w).any()
    assert np.array_equal(e["anchor"][~w], c["anchor"][~w], equal_nan=True)                    # untouched, bit for bit
    assert np.all(np.isfinite(e["anchor"][w]))
    assert np.array_equal(e["q_est"][:, 3:], c["q"][:, 3:]) and np.array_equal(e["v_est"][:, 3:], c["v"][:, 3:])
    assert np.array_equal(e["q_est"][:, 0:3], e["base"][:, 0:3]) and np.array_equal(e["v_est"][:, 0:3], e["base"][:, 3:6])
    assert np.array_equal(e["odo"] & 15, (c["contact"] & c["mask"]) & 15)
    assert np.array_equal(e["odo"] >> 4, (c["contact"] & c["mask"] & ~c["odo"]) & 15)
    # a second call on what the first left: every trusted foot has its anchor, so no anchor word moves and no foot is "new"
    e2 = R.estimate(P, c["dt"], flat_model, c["q"], c["v"], c["contact"], c["mask"], c["normals"], c["height"], e["base"], e["anchor"], e["odo"])
    assert np.array_equal(e2["anchor"], e["anchor"], equal_nan=True) and np.all(e2["odo"] >> 4 == 0) and np.array_equal(e2["odo"] & 15, e["odo"] & 15)
    if planes:                                                                                  # a new anchor lies on its plane
        nr, x = c["normals"].reshape(n, 4, 3), e["anchor"].reshape(n, 4, 3)
        gap = (nr * x).sum(2) - c["height"]
        assert np.abs(gap[e["new"]]).max() < 1e-12
    # cnt = 0: the velocity is kept, the position is dead reckoning
    idle = ~e["S"].any(1)
    assert idle.any() and np.array_equal(e["base"][idle, 3:6], c["base"][idle, 3:6])
    assert np.array_equal(e["base"][idle, 0:3], c["base"][idle, 0:3] + c["dt"] * c["base"][idle, 3:6])


def test_law_measures_a_trunk_that_moves_over_planted_feet(flat_model, total_mass):
    """What the law is for: four feet planted at known points, the trunk moving with a known velocity (the joint rates are those that keep the feet
    where they are).  With a_v = a_p = 1 one call returns the velocity and the position, whatever base holds."""
    from tests import swing_ref as SR
    n = 8
    c = R.branch_case(flat_model, total_mass, n, rank=3)
    rng = np.random.default_rng(7)
    q, v = c["q"].copy(), np.zeros((n, 18))
    q[:, 0:3] = rng.uniform(-1, 1, (n, 3))
    v[:, 0:6] = rng.uniform(-0.3, 0.3, (n, 6))
    anchor = np.zeros((n, 12))
    for k in range(4):
        K = SR.foot_kin(flat_model, k, q, v)
        anchor[:, 3 * k:3 * k + 3] = K["pf"]
        # J_l qd = -(foot velocity with the joints at rest)
        qd = np.linalg.solve(K["Jl"], -K["Jv"][:, :, None])[:, :, 0]
        for col, j in enumerate(K["joints"]):
            v[:, 6 + j] = qd[:, col]
    for k in range(4):
        assert np.abs(SR.foot_kin(flat_model, k, q, v)["Jv"]).max() < 1e-12
    qs, vs = q.copy(), v.copy()
    qs[:, 0:3], vs[:, 0:3] = np.nan, np.nan
    word = np.full(n, 15, np.int32)
    e = R.estimate(R.params(a_v=1.0, a_p=1.0), 0.0, flat_model, qs, vs, word, word, None, None, rng.uniform(-1, 1, (n, 6)), anchor, word)
    assert np.abs(e["base"][:, 0:3] - q[:, 0:3]).max() < 1e-12 and np.abs(e["base"][:, 3:6] - v[:, 0:3]).max() < 1e-12


def test_f32_errors_are_the_recorded_ones(flat_model, total_mass):
    got = R.f32_errors(flat_model, total_mass)
    print("float32 against float64:", got)
    for key, val in got.items():
        assert val <= R.F32_ERR[key] and val >= 0.25 * R.F32_ERR[key], (key, val)


def _loops(flat_model, oracle, sensed, planes=True):
    _, true = R.cpu_walk(flat_model, oracle, sensed, estimated=False)
    _, est = R.cpu_walk(flat_model, oracle, sensed, planes)
    return true, est


@pytest.mark.parametrize("sensed", ["estimate", "plant"])
def test_walking_loop_on_the_estimated_base_state(flat_model, oracle, sensed):
    """The controller links see q_est, v_est only (the law's inputs carry NaN in the base rows); the plant keeps the truth.  Every QP status is 0, and
    forward travel, base height and the estimate's error stay within the recorded bands of the true-state loop on the same case."""
    true, est = _loops(flat_model, oracle, sensed)
    assert true["status_ok"] and est["status_ok"]
    ft, fe = R.figures(true), R.figures(est)
    dtravel, dz = np.abs(fe["travel"] - ft["travel"]).max(), np.abs(fe["base_z"] - ft["base_z"]).max()
    print("%s: true travel %s z %s | estimated travel %s z %s | d travel %.4g d z %.4g | worst |p^ - p| %s rms v error %s" % (
        sensed, ft["travel"], ft["base_z"], fe["travel"], fe["base_z"], dtravel, dz, fe["perr"], fe["vrms"]))
    assert np.all(ft["travel"] > 0.045) and np.all(fe["travel"] > 0.02)              # both walk forward
    for got, band in ((dtravel, R.TRAVEL_BAND[sensed]), (dz, R.BASE_Z_BAND[sensed])):
        assert band / 4 <= got <= band, (got, band)
    for c in range(3):
        assert R.PERR_BAND[sensed][c] / 4 <= fe["perr"][c] <= R.PERR_BAND[sensed][c], (c, fe["perr"])
    # the estimate reads high by about one penetration depth (m g / (2 k_n) = 5 mm): bounded, not drifting
    zerr = est["perr"][-128:, :, 2].mean(0)
    assert np.all(zerr > 2e-3) and np.all(zerr < 8e-3), zerr
    # anchors come and go with the gait: every foot was anchored anew more than once
    assert all(int((((est["odos"] >> (4 + k)) & 1).sum(0) > 1).all()) for k in range(4))


@pytest.mark.parametrize("sensed", ["estimate", "plant"])
def test_without_planes_the_height_drifts(flat_model, oracle, sensed):
    _, est = _loops(flat_model, oracle, sensed)
    _, bare = _loops(flat_model, oracle, sensed, planes=False)
    assert bare["status_ok"]
    z_with, z_bare = R.figures(est)["perr"][2], R.figures(bare)["perr"][2]
    end_with, end_bare = est["perr"][-128:, :, 2].mean(0), bare["perr"][-128:, :, 2].mean(0)
    print("%s: worst z error %.4g with planes, %.4g without; mean of the last 128 ticks %s / %s" % (sensed, z_with, z_bare, end_with, end_bare))
    assert z_bare > R.NO_PLANES_Z * z_with and np.all(end_bare > 2 * end_with)


def test_raw_odometry_does_not_pass(flat_model, oracle):
    """a_v = a_p = 1 (no blend): the velocity estimate takes every impact and every sliding foot at face value.  The yardstick is 1 m/s, ten times
    the commanded speed: the raw estimate's worst error lies beyond it, the blended one's below."""
    case = R.walk_case(flat_model, oracle)
    raw = R.closed_loop(flat_model, oracle, case, P=R.params(a_v=1.0, a_p=1.0), ticks=256)
    _, est = R.cpu_walk(flat_model, oracle)
    print("worst |v^ - v|: raw %.3g, defaults %.3g m/s" % (np.abs(raw["verr"]).max(), np.abs(est["verr"]).max()))
    assert np.abs(raw["verr"]).max() > 1.0 > np.abs(est["verr"]).max()


def test_estimated_walking_loop_sensitivity(flat_model, oracle):
    case, est = R.cpu_walk(flat_model, oracle)
    bumped = R.closed_loop(flat_model, oracle, case, q0=case["q"] * (1 + 1e-12))
    aq, av = relerr(bumped["q"], est["q"]) / 1e-12, relerr(bumped["v"], est["v"]) / 1e-12
    print("amplification of a 1e-12 perturbation: q %.3g v %.3g" % (aq, av))
    assert np.array_equal(bumped["masks"], est["masks"])
    assert aq <= R.WALK_AMPLIFICATION["q"] and av <= R.WALK_AMPLIFICATION["v"]
