"""CPU: the referee of tests/test_gpu_walk_edges.py on exactly that file's inputs (tests/walk_edges.py) -- the ground plant, stiction, contact sensing,
leg odometry and the terrain feet on wide states, planes over the whole sphere and mu from 0.05 to 1.5.  The cases are what they claim to be (every
branch taken, every decision clear of its switching point in both scalar types, negative and singular leg determinants present, skip sets under their
cap); every law agrees with its second implementation in float64; four deliberately wrong laws are each CAUGHT on the wide cases (and two of them pass
the committed narrow cases, which is why the wide ones exist); and what float32 costs on these inputs is measured HERE, so that the GPU file's fp32
gates are not taken from the code under test."""
import numpy as np
import pytest

from tests import contact_ref as CR, envelope as E, ground_ref as GND, limit_ref, odom_ref as OD, stick_ref as ST, swing_ref as SR, terrain_ref as TR, \
    walk_edges as WE
from tests.util import elementwise_excess, unpack_M

GATE_MARGIN = 8.0       # the GPU file's fp32 gates are this x the F32_* figures


@pytest.fixture(scope="module")
def total_mass(flat_model):
    return float(np.sum(flat_model["mass"]))


def _beyond(a, b, f32_err):
    """the difference of two results would fail BOTH gates of the GPU file: fp32 (GATE_MARGIN x the figure, of the largest entry) and fp64
    (util.elementwise_excess at the standing tolerances)"""
    return WE.rel(a, b) > GATE_MARGIN * f32_err and elementwise_excess(a, b) > 1.0


def _within(a, b):
    """... would pass both"""
    return elementwise_excess(a, b) <= 1.0


# ---- the inputs are what they claim to be
def test_wide_states_and_planes(flat_model, total_mass):
    n = 130
    B = WE.wide_states(flat_model, total_mass, n, rank=n)
    W = E.wide_batch(4, n, total_mass, rank=200 + n)
    assert np.array_equal(B["q"], W["q"]) and np.array_equal(B["v"], W["v"])             # envelope's states, untouched
    nrm = B["normals"].reshape(n, 4, 3)
    assert np.abs(np.linalg.norm(nrm, axis=2) - 1.0).max() < 1e-15                       # unit
    assert (nrm[..., 2] < 0).mean() > 0.2 and (np.abs(nrm[..., 0]) >= 0.9).mean() > 0.3  # downward; the e_y arm of the contact frame
    assert np.degrees(np.arccos(np.abs(nrm[..., 2]))).max() > 80
    assert B["mu"].min() < 0.1 and B["mu"].max() > 1.4 and B["mu"].min() >= 0.05 and B["mu"].max() <= 1.5
    assert np.abs(B["q"][:, 0:2]).max() > 45
    S = WE.wide_states(flat_model, total_mass, n, rank=n, quat_scale=True)
    ln = np.linalg.norm(S["q"][:, 3:7], axis=1)
    assert ln.min() < 0.6 and ln.max() > 1.8 and ln.min() >= 0.5 and ln.max() <= 2.0
    assert np.allclose(S["q"][:5, 3:7] / ln[:5, None], E.EDGE_QUATS, atol=1e-15)
    # the redraw for the builder's solve touches joints of ill-conditioned legs only
    G = WE.wide_states(flat_model, total_mass, n, rank=n, solve_cond_max=WE.SOLVE_COND_MAX)
    was = WE.leg_conds(flat_model, W["q"])
    legs = limit_ref.leg_joints(flat_model)
    for k in range(4):
        cols = [7 + j for j in legs[k]]
        moved = np.any(G["q"][:, cols] != W["q"][:, cols], axis=1)
        assert np.array_equal(moved, ~(was[:, k] <= WE.SOLVE_COND_MAX))
    assert WE.leg_conds(flat_model, G["q"]).max() <= WE.SOLVE_COND_MAX
    print("legs redrawn for the ground cases: %.1f %%" % (100 * (~(was <= WE.SOLVE_COND_MAX)).mean()))


@pytest.mark.parametrize("n", WE.SIZES)
def test_ground_and_stick_cases_take_every_branch_with_clear_decisions(flat_model, total_mass, n):
    P = GND.params()
    for stick in (False, True):
        c = (WE.wide_stick_case if stick else WE.wide_ground_case)(flat_model, total_mass, n)
        (_, _, g64), (_, _, g32) = c["ref64"], c["ref32"]
        if stick:
            assert ST.branches_taken(g64) == ST.ALL_BRANCHES
        else:
            assert GND.branches_taken(P, g64) == GND.ALL_BRANCHES
        m = GND.margins(P, g64)
        assert all(x >= 1.0 for x in m.values()), m                       # ground_ref.MARGIN and GAP_MARGIN
        assert not WE.unsafe_feet(P, g64, g32).any()
        assert np.array_equal(g32["contact"], g64["contact"]) and (not stick or np.array_equal(g32["stick"], g64["stick"]))
        # where the case lives: 50 m out, planes over the sphere, anchors around the feet
        assert np.abs(c["q"][:, 0:2]).max() > 40 and np.abs(c["height"]).max() > 20
        assert (c["normals"].reshape(n, 4, 3)[..., 2] < 0).any()
        if stick:
            w = g64["had"] & g64["loaded"]
            assert np.abs(c["anchor"].reshape(n, 4, 3)[w] - g64["pf"][w]).max() < 0.02 and np.abs(c["anchor"].reshape(n, 4, 3)[w]).max() > 40
        gap32 = float(np.abs(g32["gap"].astype(np.float64) - g64["gap"]).max())
        print("%s n=%d: margins %s; float32 gap error %.3g m (POS_NOISE32 %.3g, GAP_MARGIN %.3g)"
              % ("stick" if stick else "ground", n, {k: round(x, 2) for k, x in m.items()}, gap32, WE.POS_NOISE32, GND.GAP_MARGIN))
        assert gap32 < WE.POS_NOISE32 < GND.GAP_MARGIN / 4


@pytest.mark.parametrize("n", WE.SIZES)
def test_contact_case_has_negative_and_singular_determinants(flat_model, total_mass, n):
    P = CR.params()
    c = WE.wide_contact_case(flat_model, total_mass, n)
    fig = WE.contact_figures(flat_model, c)
    skip = c["skip"]
    print("contact n=%d: det < 0 on %.1f %% of the regular legs, %.1f %% singular (per foot %s), largest cond of a regular leg %.1f, %.2f %% skipped"
          % (n, 100 * fig["neg"], 100 * fig["singular"], fig["per_foot"], fig["cond"], 100 * skip.mean()))
    assert fig["neg"] >= 1.0 / 3.0
    assert np.all(fig["per_foot"] >= 1)
    assert fig["cond"] > 2 * CR.COND_MAX                                  # beyond anything the committed case has
    assert skip.mean() <= WE.SKIP_CAP
    assert CR.branches_taken(P, c["e64"]) == CR.ALL_BRANCHES
    keep = ~skip
    assert np.array_equal(WE._bits(c["e64"]["contact"])[keep], WE._bits(c["e32"]["contact"])[keep])
    assert np.array_equal(WE._bits(c["e64"]["singular"])[keep], WE._bits(c["e32"]["singular"])[keep])
    assert not (WE.contact_skip(P, c["e64"], CR.MARGIN64) & keep).any() and not (WE.contact_skip(P, c["e32"], CR.MARGIN32) & keep).any()
    # the committed case: |det| in the standing posture's narrow band, cond <= COND_MAX.  (Its determinants are NOT all positive: the legs of one body
    # side are mirror images of the other's, so half of them are negative there too -- the sign is met by the committed case, the size is not.)
    nar = CR.branch_case(flat_model, 64, rank=64)
    e = WE.run_contact(P, nar, limit_ref.leg_joints(flat_model))
    reg = nar["kinds"] != 6
    assert 1.5e-2 < np.abs(e["det"][reg]).min() and np.abs(e["det"][reg]).max() < 5e-2 and CR.worst_cond(nar, limit_ref.leg_joints(flat_model)) <= CR.COND_MAX
    print("committed contact case: det < 0 on %.1f %% of the regular legs, |det| %.3g .. %.3g" % (100 * (e["det"][reg] < 0).mean(), np.abs(e["det"][reg]).min(),
                                                                                               np.abs(e["det"][reg]).max()))
    assert 0.3 < (e["det"][reg] < 0).mean() < 0.7


@pytest.mark.parametrize("n", WE.SIZES)
def test_odom_case_takes_every_branch(flat_model, total_mass, n):
    for planes in (True, False):
        c = WE.wide_odom_case(flat_model, total_mass, n, planes=planes)
        e = c["ref64"]
        for lo in range(0, n - 15, 16):
            assert OD.branches_taken({key: e[key][lo:lo + 16] for key in ("S", "A", "had")}) == OD.ALL_BRANCHES, lo
        assert np.all(np.isfinite(e["base"])) and np.all(np.isfinite(e["anchor"][OD.written(e)]))
        assert np.all(np.isnan(c["q"][:, 0:3])) and np.all(np.isnan(c["v"][:, 0:3]))
        ln = np.linalg.norm(c["q"][:, 3:7], axis=1)
        assert ln.min() < 0.7 and ln.max() > 1.5                               # attitudes far from unit length
        assert np.abs(c["base"][:, 0:2]).max() > 40
        lever, _ = OD.leg_terms(flat_model, c["q"], c["v"])
        had = OD._bits(c["odo"])
        foot = c["base"][:, None, 0:3] + lever
        assert np.abs(c["anchor"].reshape(n, 4, 3)[had] - foot[had]).max() < 0.05
        if planes:
            gap = (c["normals"].reshape(n, 4, 3) * foot).sum(2) - c["height"]
            assert np.abs(gap).max() < 0.05                                    # every plane passes by its foot, not by the origin


@pytest.mark.parametrize("kind", WE.FEET_KINDS)
def test_feet_cases(flat_model, total_mass, kind):
    for n in WE.feet_sizes(kind):
        c = WE.wide_feet_case(flat_model, total_mass, kind, n)
        r64, r32 = c["ref64"], c["ref32"]
        assert r64["margin"] >= TR.MARGIN64 and r32["margin"] >= TR.MARGIN32
        spread = float(np.abs(r64["pf"][:, :, 0:2] - c["q"][:, None, 0:2]).max())
        print("feet %s n=%d: feet up to %.2f m from the trunk, grid %s at (%.3f, %.3f), inside %s" % (kind, n, spread, c["T"]["z"].shape, c["T"]["x0"],
                                                                                                    c["T"]["y0"], r64["inside"]))
        assert spread > 0.5 and np.array_equal(c["mask"], np.arange(n) % 16)
        assert r64["inside"] == (kind != "clamped") and r32["inside"] == r64["inside"]
        if kind == "far":
            assert np.hypot(c["T"]["x0"], c["T"]["y0"]) > 10 and np.abs(c["q"][:, 0:2]).max() > 10
        if kind == "clamped":
            nz, ny, nx = c["T"]["z"].shape
            x, y = r64["pf"][..., 0], r64["pf"][..., 1]
            xm, ym = c["T"]["x0"] + (nx - 1) * c["T"]["cell"], c["T"]["y0"] + (ny - 1) * c["T"]["cell"]
            assert (x < c["T"]["x0"]).any() and (x > xm).any() and (y < c["T"]["y0"]).any() and (y > ym).any()       # beyond every edge


@pytest.mark.parametrize("n", WE.SIZES)
def test_gait_and_ramp_cases(flat_model, total_mass, n):
    from tests import gait_ref as GR
    c = WE.wide_gait_case(flat_model, total_mass, n)
    g = c["gait"]
    assert GR.branches_taken(GR.params(flat_model), 1e-3, [g]) == GR.ALL_BRANCHES
    assert np.array_equal(c["odom"]["q"][:, 3:], g["q"][:, 3:]) and np.all(np.isnan(c["odom"]["q"][:, 0:3]))
    assert np.abs(c["odom"]["base"][:, 0:3] - g["q"][:, 0:3]).max() <= 0.01 and np.abs(g["q"][:, 0:2]).max() > 40
    F = TR.feet(flat_model, c["T"], c["q_near"], None, None, c["tile"])
    assert F["inside"] and F["margin"] >= TR.MARGIN64
    r = WE.ramp_case(flat_model, total_mass, n)
    F, G = r["ref64"]["feet"], r["ref64"]["ground"]
    assert F["inside"] and np.abs(np.abs(F["normals"][:, 0::3]) - 2 / np.sqrt(5)).max() < 1e-12         # every plane is the ramp's
    own = G["gap"][np.arange(n), np.arange(n) % 4]
    assert np.abs(own + WE.RAMP_DIP / np.sqrt(5)).max() < 1e-9                                           # the chosen foot: 2.2 mm inside, 45 N
    assert (G["fn"] == 0).mean() > 0.2 and (G["fn"] > 1e3).mean() > 0.2                                 # the others: in the air, and deep inside
    print("ramp n=%d: %.2f %% of the feet skipped, f_n up to %.3g N" % (n, 100 * r["skip"].mean(), G["fn"].max()))
    assert r["skip"].mean() <= WE.SKIP_CAP
    keep = ~r["skip"]
    assert np.array_equal(WE._bits(G["contact"])[keep], WE._bits(r["ref32"]["ground"]["contact"])[keep])


def test_cost_grids_have_partial_workgroups_that_are_not_the_first():
    TX, TY = 32, 8        # terrain_cost_kernel's tile
    for name in WE.COST_GRIDS:
        T = WE.cost_grid(name)
        nz, ny, nx = T["z"].shape
        assert T["z"].dtype == np.float64 and np.array_equal(T["z"] * 1024, np.rint(T["z"] * 1024))
        assert np.array_equal(T["z"].astype(np.float32), T["z"])
        print("cost grid %s: %d x %d workgroups per tile, last one holds %d x %d nodes" % (name, -(-nx // TX), -(-ny // TY), (nx - 1) % TX + 1, (ny - 1) % TY + 1))
    nz, ny, nx = WE.cost_grid("70x19x2")["z"].shape
    assert (nz, nx % TX, ny % TY, nx // TX, ny // TY) == (2, 6, 3, 2, 2)
    assert WE.cost_grid("33x9")["z"].shape == (1, 9, 33) and WE.cost_grid("31x7")["z"].shape == (1, 7, 31)


# ---- each law against its second implementation, float64
@pytest.mark.parametrize("n", WE.SIZES)
def test_laws_agree_with_their_second_implementations(flat_model, oracle, total_mass, n):
    legs = limit_ref.leg_joints(flat_model)
    # contact: the adjugate form against numpy's solve, the gate of tests/test_contact_oracle.py
    c = WE.wide_contact_case(flat_model, total_mass, n)
    P = CR.params()
    e, b = c["e64"], CR.estimate_brute(P, c["Jc"], c["r"], c["f_prev"], c["normals"], c["contact"], legs)
    assert np.array_equal(e["contact"], b["contact"]) and np.array_equal(e["singular"], b["singular"])
    ef, en = np.abs(e["f_est"] - b["f_est"]).max(), np.abs(e["fn"] - b["fn"]).max()
    print("contact n=%d: estimate against estimate_brute f_est %.3g fn %.3g" % (n, ef, en))
    assert ef < 1e-11 and en < 1e-11
    # odometry: the vectorised law against the loop, bit for bit as tests/test_odom_oracle.py holds them
    for planes in (True, False):
        c = WE.wide_odom_case(flat_model, total_mass, n, planes=planes)
        a, b = c["ref64"], OD.run(OD.params(), flat_model, c, fn=OD.estimate_loop)
        for key in ("base", "anchor", "odo", "q_est", "v_est"):
            assert np.array_equal(a[key], b[key], equal_nan=True), key
    # ground and stiction: the plant step of ground_ref against envelope.integrate_ref, 1e-12 of the largest entry
    for stick in (False, True):
        c = (WE.wide_stick_case if stick else WE.wide_ground_case)(flat_model, total_mass, n)
        q64, v64, g = c["ref64"]
        M = unpack_M(c["dyn"]["M"])
        a = E.integrate_ref(WE.DT, M, c["dyn"]["h"], c["dyn"]["Jc"], c["tau"], g["f_gr"], c["tau_ext"], c["q"], c["v"])
        b = GND.plant_step(WE.DT, M, c["dyn"]["h"], c["dyn"]["Jc"], c["tau"], g["f_gr"], c["tau_ext"], c["q"], c["v"])
        assert np.array_equal(a[0], q64) and np.array_equal(a[1], v64)          # (integrate_ground in float64 IS integrate_ref with f = f_gr)
        eq, ev = WE.rel(b[0], a[0]), WE.rel(b[1], a[1])
        print("%s n=%d: plant_step against integrate_ref q %.3g v %.3g" % ("stick" if stick else "ground", n, eq, ev))
        assert eq < 1e-12 and ev < 1e-12
        # ... and the leg kinematics the cases were built on: swing_ref.foot_kin against the oracle's pf / Jc.  tests/test_swing_oracle.py holds the
        # pair to 1e-14 absolute near the origin; J_leg (no position in it) keeps that figure, p_f (an ulp of 50 m is 7e-15) and J v (joint rates of
        # up to 100 rad/s) are held to 1e-12 of the largest entry
        d = oracle.dynamics(c["q"], c["v"])
        Jc = d["Jc"].reshape(n, 12, 18)
        for k in range(4):
            K = SR.foot_kin(flat_model, k, c["q"], c["v"])
            assert WE.rel(K["pf"], d["pf"][:, 3 * k:3 * k + 3]) < 1e-12
            assert np.abs(K["Jl"] - Jc[:, 3 * k:3 * k + 3][:, :, [6 + j for j in K["joints"]]]).max() < 1e-14
            assert WE.rel(K["Jv"], np.einsum("nij,nj->ni", Jc[:, 3 * k:3 * k + 3], c["v"])) < 1e-12
            assert [j for j in K["joints"]] == list(legs[k])


# ---- the cases can fail: four wrong laws
def _no_abs(P, c, e, legs):
    """contact_ref.estimate with `det > det_min` in place of `|det| > det_min`: a leg with det < -det_min is taken for singular -- df = 0, the bit kept"""
    out = {k: np.array(x) for k, x in e.items()}
    n = len(out["contact"])
    for k in range(4):
        lost = e["det"][:, k] < -P["det_min"]
        fp = c["f_prev"][:, 3 * k:3 * k + 3]
        out["f_est"][lost, 3 * k:3 * k + 3] = fp[lost]
        out["fn"][lost, k] = (c["normals"][:, 3 * k:3 * k + 3] * fp).sum(1)[lost]
        was = (e["prev"] >> k) & 1
        out["contact"][lost] = (out["contact"][lost] & ~np.int32(1 << k)) | (was[lost] << k)
        out["singular"][lost] |= 1 << k
    return out


def test_mutation_det_without_abs_is_caught(flat_model, total_mass):
    """Caught on the wide case -- and on the committed narrow case as well: the mirrored legs of one body side have det < 0 in the standing posture
    too, so a kernel that tested `det > det_min` never passed tests/test_gpu_contact.py either.  What the wide case adds for this law is |det| down to
    det_min, legs that are singular by themselves and cond(J_leg) of 157 where the committed case has 3.7."""
    P, legs = CR.params(), limit_ref.leg_joints(flat_model)
    n = 65
    c = WE.wide_contact_case(flat_model, total_mass, n)
    bad = _no_abs(P, c, c["e64"], legs)
    keep = ~c["skip"]
    assert (WE._bits(bad["singular"]) != WE._bits(c["e64"]["singular"]))[keep].any()
    assert (WE._bits(bad["contact"]) != WE._bits(c["e64"]["contact"]))[keep].any()
    assert _beyond(bad["f_est"], c["e64"]["f_est"], WE.F32_CONTACT["f_est"]) and _beyond(bad["fn"], c["e64"]["fn"], WE.F32_CONTACT["fn"])
    nar = CR.branch_case(flat_model, 64, rank=64)
    e = WE.run_contact(P, nar, legs)
    also = _no_abs(P, nar, e, legs)
    assert not np.array_equal(also["singular"], e["singular"]) and WE.rel(also["f_est"], e["f_est"]) > CR.F32_GATE


def test_mutation_mu_rounded_to_three_values_is_caught(flat_model, total_mass):
    P, legs = GND.params(), limit_ref.leg_joints(flat_model)
    rounded = lambda mu: np.array([0.4, 0.6, 0.8])[np.abs(mu[..., None] - np.array([0.4, 0.6, 0.8])).argmin(-1)]
    c = WE.wide_ground_case(flat_model, total_mass, 65)
    g = c["ref64"][2]
    bad = GND.ground_force(P, c["q"], c["v"], c["dyn"]["Jc"], c["normals"], c["height"], rounded(c["mu"]), legs)
    assert _beyond(bad["f_gr"], g["f_gr"], WE.F32_GROUND["f_gr"])
    s = WE.wide_stick_case(flat_model, total_mass, 65)
    gs = s["ref64"][2]
    bad = ST.stick_force(P, ST.DEFAULT_KT, s["q"], s["v"], s["dyn"]["Jc"], s["normals"], s["height"], rounded(s["mu"]), s["anchor"], s["stick"], legs)
    assert _beyond(bad["f_gr"], gs["f_gr"], WE.F32_STICK["f_gr"]) and not np.array_equal(bad["stick"], gs["stick"])
    nar = GND.branch_case(flat_model, total_mass, 33, rank=33)
    a = GND.ground_force(P, nar["q"], nar["v"], nar["dyn"]["Jc"], nar["normals"], nar["height"], nar["mu"], legs)
    b = GND.ground_force(P, nar["q"], nar["v"], nar["dyn"]["Jc"], nar["normals"], nar["height"], rounded(nar["mu"]), legs)
    assert np.array_equal(a["f_gr"], b["f_gr"])                           # the committed case has no other mu


def test_mutation_no_quaternion_normalisation_is_caught_only_on_the_wide_case(flat_model, total_mass, monkeypatch):
    n = 65
    c = WE.wide_odom_case(flat_model, total_mass, n)
    nar = OD.branch_case(flat_model, total_mass, 64, rank=64)
    good_nar = OD.run(OD.params(), flat_model, nar)
    with monkeypatch.context() as m:
        m.setattr(SR, "_quat_R", _quat_R_raw)      # the rotation formula on the quaternion as it comes
        bad, bad_nar = OD.run(OD.params(), flat_model, c), OD.run(OD.params(), flat_model, nar)
    e = c["ref64"]
    w = OD.written(e)
    assert _beyond(bad["base"][:, 0:3], e["base"][:, 0:3], WE.F32_ODOM["p"]) and _beyond(bad["base"][:, 3:6], e["base"][:, 3:6], WE.F32_ODOM["v"])
    assert _beyond(bad["anchor"][w], e["anchor"][w], WE.F32_ODOM["anchor"])
    wn = OD.written(good_nar)
    assert _within(bad_nar["base"], good_nar["base"]) and _within(bad_nar["anchor"][wn], good_nar["anchor"][wn])     # unit attitudes cannot tell


def _quat_R_raw(qq):
    dt = qq.dtype.type
    x, y, z, w = qq.T
    one, two = dt(1), dt(2)
    return np.stack([np.stack([one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)], 1),
                     np.stack([two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)], 1),
                     np.stack([two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)], 1)], 1)


def test_mutation_plane_drop_along_e_z_is_caught(flat_model, total_mass):
    n = 65
    c = WE.wide_odom_case(flat_model, total_mass, n)
    e = c["ref64"]
    w = OD.written(e)
    ez = dict(c, normals=np.tile([0.0, 0.0, 1.0], (n, 4)))
    bad = OD.run(OD.params(), flat_model, ez)
    assert np.array_equal(bad["odo"], e["odo"]) and np.array_equal(bad["base"], e["base"])      # the drop reaches the new anchors alone
    assert _beyond(bad["anchor"][w], e["anchor"][w], WE.F32_ODOM["anchor"])


# ---- what float32 costs
def _check(name, measured, committed):
    print("%s: measured %s, committed %s" % (name, {k: "%.2g" % x for k, x in measured.items()}, committed))
    assert set(measured) == set(committed)
    for k, x in measured.items():
        assert x <= committed[k] <= 2 * max(x, WE.F32_FLOOR / 2), (name, k, x, committed[k])


def test_f32_figures(flat_model, total_mass):
    _check("F32_GROUND", WE.f32_plant_errors(flat_model, total_mass, False), WE.F32_GROUND)
    _check("F32_STICK", WE.f32_plant_errors(flat_model, total_mass, True), WE.F32_STICK)
    _check("F32_CONTACT", WE.f32_contact_errors(flat_model, total_mass), WE.F32_CONTACT)
    _check("F32_ODOM", WE.f32_odom_errors(flat_model, total_mass), WE.F32_ODOM)
    for kind in WE.FEET_KINDS:
        _check("F32_FEET[%s]" % kind, WE.f32_feet_errors(flat_model, total_mass, kind), WE.F32_FEET[kind])
    _check("F32_RAMP", WE.f32_ramp_errors(flat_model, total_mass), WE.F32_RAMP)
