"""CPU: the referee of tests/test_gpu_contact_edges.py on exactly that file's inputs (tests/contact_edges.py) -- contact words outside what
synth.make_batch draws: all sixteen stance masks, normals over the whole sphere with a third of the feet on the e_y arm of the contact frame, friction from
0.05 to 1.5, whole workgroups and whole batches in flight.  The inputs are what they claim to be; the oracle's QP assembly agrees with the numpy second
implementation on them and its solutions meet the KKT conditions (the textbook primal solver of crosscheck_np stalls on some of these QPs, so it is no
referee here); every case meets its CONDITIONS (conditions of the inputs: a seed that misses one is changed, never the threshold); a contact frame that
always takes e_x moves the reference far beyond every gate; and what float32 costs on these inputs is measured HERE and pinned in
tests/contact_edges.py, so that no GPU gate is taken from the code under test."""
import numpy as np
import pytest

from oracle import crosscheck_np as X, oracle_py as O
from tests import contact_edges as CE, envelope as E, limit_ref, variants as V
from tests.util import _obs_state, relerr
from wbc_quadruped_dob_amd import synth

F32_TOL, F32_DYN, F32_OBS = 5e-4, 1e-4, (1e-4, 2e-3)       # the project's fp32 gates: tau and f; dynamics and rollout states; observer integ / r
TIGHT64 = 1e-9
ROWS = {c[0]: c for c in E.TICK_CASES}


@pytest.fixture(scope="module")
def total_mass(flat_model):
    return float(np.sum(flat_model["mass"]))


def _cases():
    """(id, row, flight) of every tick the GPU file runs: all of envelope.TICK_CASES, and CE.FLIGHT_ROWS with a block in flight and all in flight"""
    out = [(c[0], c, None) for c in E.TICK_CASES]
    for fl in ("block", "all"):
        out += [("%s-%s" % (cid, fl), ROWS[cid], fl) for cid in CE.FLIGHT_ROWS if fl == "all" or ROWS[cid][4] >= CE.FLIGHT_BLOCK[1]]
    return out


def test_the_flight_block_runs_on_all_seven_rows():
    assert len(_cases()) == len(E.TICK_CASES) + 2 * len(CE.FLIGHT_ROWS)
    assert max(c[4] for c in E.TICK_CASES) == 258


def test_contact_batch_is_what_it_claims(total_mass):
    n = 258
    for cfg in (2, 3, 4):
        narrow = synth.make_batch(cfg, n, total_mass, rank=n)
        B = CE.contact_batch(cfg, n, total_mass, rank=n)
        # what make_batch reaches
        assert np.abs(CE.unit_normals(narrow["normals"])[..., 0]).max() < 0.26 and set(np.unique(narrow["mu"])) <= {0.4, 0.6, 0.8}
        assert 0 not in set(narrow["mask"]) and len(set(narrow["mask"])) <= 9
        # masks: every 16 consecutive states carry all 16 patterns; state 0 is a single foot
        assert B["mask"][0] == 0b0100 and B["mask"].dtype == np.int32
        for g in range(0, n - 15):
            assert set(B["mask"][g:g + 16]) == set(range(16))
        # normals: a third on the e_y arm with both signs of n_x, downward normals, lengths 0.3 ... 3, nothing within TIE of the switch
        u = CE.unit_normals(B["normals"])
        steep = CE.steep_feet(B["normals"])
        assert 0.3 < steep.mean() < 0.5 and (u[..., 0][steep] > 0).any() and (u[..., 0][steep] < 0).any()
        assert (u[..., 2] < -0.5).mean() > 0.1 and (np.abs(u[..., 1]) > 0.9).any()
        ln = np.linalg.norm(B["normals"].reshape(n, 4, 3), axis=2)
        assert 0.3 <= ln.min() < 0.4 and 2.8 < ln.max() <= 3.0
        assert CE.tie_distance(B["normals"]) >= CE.TIE
        # friction: all five values
        assert set(np.unique(B["mu"])) == set(CE.MU)
        # everything else is make_batch's
        for key in narrow:
            if key not in ("mask", "normals", "mu", "w_des"):
                assert np.array_equal(B[key], narrow[key]), key
        assert np.array_equal(B["w_des"][:, 3:], narrow["w_des"][:, 3:])
        assert np.allclose(B["w_des"][:, 0:3], narrow["w_des"][:, 0:3] * np.asarray(V.FORCE_SCALE)[np.arange(n) % 4, None], rtol=0, atol=0)
        # flight
        blk, al = CE.contact_batch(cfg, n, total_mass, rank=n, flight="block"), CE.contact_batch(cfg, n, total_mass, rank=n, flight="all")
        assert np.all(blk["mask"][16:32] == 0) and np.array_equal(np.delete(blk["mask"], np.s_[16:32]), np.delete(B["mask"], np.s_[16:32])) and not al["mask"].any()
        for key in ("normals", "mu", "w_des", "q"):
            assert np.array_equal(blk[key], B[key]) and np.array_equal(al[key], B[key])
        # the warm test's second batch: other masks, everything else the same
        other = CE.contact_batch(cfg, n, total_mass, rank=n, mask_offset=9)
        assert (other["mask"] != B["mask"]).all() and np.array_equal(other["normals"], B["normals"]) and np.array_equal(other["mu"], B["mu"])
    with pytest.raises(AssertionError):
        CE.contact_batch(4, 17, total_mass, flight="block")


@pytest.mark.parametrize("cid", ["fused", "tile-f64-obs0", "two-lane", "two-qptile64"])
def test_assembly_matches_numpy_and_the_solutions_meet_kkt(oracle, total_mass, cid):
    """tests/test_qp_oracle.py's assembly tolerances (H 1e-13, g 1e-12, C 1e-14, relative to the largest entry where that exceeds 1: S reaches 30 and
    the desired force 650 N here; d exactly) on the first 48 states -- three times every mask, steep feet among them -- and the KKT gates of
    test_gi_matches_primal_active_set_and_kkt on the oracle's own solution, which is also the f of oracle.step"""
    row = ROWS[cid]
    B, P = CE.tick_inputs(row, total_mass)
    P = dict(P, observer_order=0, qp_tol=1e-9)
    ref = oracle.step(P, B["q"], B["v"], B["w_des"], B["vdot_des"], B["normals"], B["mu"], B["mask"], B["tau_prev"], B["f_prev"], nthreads=8)
    pf = oracle.dynamics(B["q"], B["v"])["pf"]
    m = min(48, row[4])
    steep = (CE.steep_feet(B["normals"]) & CE.stance(B["mask"]))[:m].any(axis=1)
    assert set(B["mask"][:m]) == set(range(16)) and steep.sum() >= 16
    big = lambda a: max(1.0, float(np.abs(a).max())) if a.size else 1.0
    for s in range(m):
        mask = int(B["mask"][s])
        H, g, C, d = O.qp_assemble(P, 4, mask, B["q"][s, 0:3], pf[s], B["normals"][s], B["mu"][s], B["w_des"][s])
        Hn, gn, Cn, dn, st = X.qp_assemble(P, mask, B["q"][s, 0:3], pf[s].reshape(4, 3), B["normals"][s].reshape(4, 3), B["mu"][s], B["w_des"][s])
        if not mask:
            assert H.size == 0 and not ref["f"][s].any() and ref["iters"][s] == 0 and ref["status"][s] == 0
            continue
        np.testing.assert_allclose(H, Hn, rtol=0, atol=1e-13 * big(Hn))
        np.testing.assert_allclose(g, gn, rtol=0, atol=1e-12 * big(gn))
        np.testing.assert_allclose(C, Cn, rtol=0, atol=1e-14 * big(Cn))
        np.testing.assert_allclose(d, dn, rtol=0, atol=0)
        x, lam, status, iters = O.qp_solve(H, g, C, d)
        assert status == 0
        stat, feas, dual, comp = X.kkt_residuals(H, g, C, d, x, lam)
        scale = max(1.0, np.abs(g).max())
        assert stat < 1e-9 * scale and feas < 1e-8 and dual < 1e-12 and comp < 1e-7 * scale, (s, mask, stat, feas, dual, comp)
        f = np.zeros(12)
        for i, k in enumerate(st):
            f[3 * k:3 * k + 3] = x[3 * i:3 * i + 3]
        assert relerr(ref["f"][s], f) < TIGHT64, (s, mask)


def _fp64_tick(oracle, row, total_mass, flight):
    B, P = CE.tick_inputs(row, total_mass, flight)
    ref, _, _ = CE.oracle_tick(oracle, dict(P, qp_tol=1e-9), B, "f64", _obs_state(oracle, B, "f64", row[2]))
    return B, P, ref


def test_every_tick_case_meets_its_conditions(oracle, total_mass):
    """Every tick of the GPU file, flight variants included: status 0 everywhere in both scalar types; all sixteen masks; no foot within TIE of the
    switch; at n >= 17 at least a quarter of the states with a steep stance foot that has an active friction row (per foot, from the oracle's active
    set) and fn_min and fn_max rows both seen (flight = "all" apart: no QP there, f = 0 and no iteration)."""
    for name, row, flight in _cases():
        cid, dtype, obs, cfg, n = row[:5]
        B, P, ref = _fp64_tick(oracle, row, total_mass, flight)
        r32, _, _ = CE.oracle_tick(oracle, dict(P, qp_tol=1e-3), B, "f32", _obs_state(oracle, B, "f64", obs))
        a = V.active_classes(ref["aset"], B["mask"])
        sa = CE.steep_active(ref["aset"], B["mask"], B["normals"])
        print("%-22s %s n=%-3d iterations up to %2d; steep stance foot with an active friction row %.0f %%, fn_min %.0f %%, fn_max %.0f %%; tie distance %.3f"
              % (name, CE.tick_params(cid), n, int(ref["iters"].max()), 100 * sa.mean(), 100 * a["fn_min"].mean(), 100 * a["fn_max"].mean(), CE.tie_distance(B["normals"])))
        assert np.all(ref["status"] == 0) and np.all(r32["status"] == 0), name
        assert ref["iters"].max() <= 30, (name, int(ref["iters"].max()))
        assert CE.tie_distance(B["normals"]) >= CE.TIE, name
        assert not ref["f"].reshape(n, 4, 3)[~CE.stance(B["mask"])].any() and not r32["f"].reshape(n, 4, 3)[~CE.stance(B["mask"])].any()
        fl = B["mask"] == 0
        assert not ref["f"][fl].any() and not ref["iters"][fl].any() and not r32["iters"][fl].any()
        if flight == "all":
            assert fl.all()
            continue
        if flight == "block":
            assert fl[16:32].all()
        if n >= 17:
            assert set(B["mask"]) == set(range(16)), name
            assert sa.mean() >= 0.25, (name, sa.mean())
            assert a["fn_min"].any() and a["fn_max"].any(), name


def test_a_frame_that_always_takes_e_x_cannot_pass(oracle, total_mass, monkeypatch):
    """Discriminating power.  crosscheck_np.contact_frame patched to take e_x whatever the normal (a wrong e_y arm still yields an orthonormal frame: a
    rotated pyramid, feasible), the QP assembled with it and solved by oracle_py.qp_solve: on the states with a steep stance foot that has an active
    friction row, f moves by more than 10 x the fp64 gate (1e-8 of the case's largest force) on at least a quarter, and by more than 10 x the fp32
    gate (5e-3) on at least a tenth -- in every tick case of 17 states and more."""
    right_frame = X.contact_frame

    def always_ex(n):
        n = n / np.linalg.norm(n)
        t1 = np.array([1.0, 0, 0]) - n * n[0]
        t1 /= np.linalg.norm(t1)
        return t1, np.cross(n, t1), n

    for row in E.TICK_CASES:
        cid, dtype, obs, cfg, n = row[:5]
        if n < 17:
            continue
        B, P, ref = _fp64_tick(oracle, row, total_mass, None)
        P = dict(P, qp_tol=1e-9)
        sa = np.flatnonzero(CE.steep_active(ref["aset"], B["mask"], B["normals"]))
        pf = oracle.dynamics(B["q"], B["v"])["pf"]
        fmax = max(1.0, float(np.abs(ref["f"]).max()))
        moved = np.zeros(len(sa))
        for i, s in enumerate(sa):
            sol = []
            for frame in (right_frame, always_ex):
                monkeypatch.setattr(X, "contact_frame", frame)
                # (b: the wrench this state's QP was solved for matters only through the comparison of the two frames; the observer's share is left out)
                H, g, C, d, st = X.qp_assemble(P, int(B["mask"][s]), B["q"][s, 0:3], pf[s].reshape(4, 3), B["normals"][s].reshape(4, 3), B["mu"][s], B["w_des"][s])
                x, lam, status, _ = O.qp_solve(H, g, C, d)
                assert status == 0
                sol.append(x)
            moved[i] = np.abs(sol[1] - sol[0]).max() / fmax
        monkeypatch.setattr(X, "contact_frame", right_frame)
        fine, coarse = (moved > 10 * TIGHT64).mean(), (moved > 10 * F32_TOL).mean()
        print("%-18s always e_x: of %3d states with a loaded steep foot, f moves by > 1e-8 on %.0f %%, by > 5e-3 on %.0f %% (median %.2g)"
              % (cid, len(sa), 100 * fine, 100 * coarse, np.median(moved)))
        assert fine >= 0.25 and coarse >= 0.10, (cid, fine, coarse)


def test_f32_tick_constants_are_what_the_oracle_measures(oracle, total_mass):
    """The fp32 oracle against the fp64 oracle on every tick of the GPU file (printed); contact_edges.F32_TICK pins the figures of the ones that run in
    fp32: never below the measurement, never more than twice it.  No status flip; the observer state and the dynamics outputs stay below a quarter
    of their gates, so those gates carry over unchanged."""
    fp32 = {name for name, row, _ in _cases() if row[1] == "f32"}
    assert set(CE.F32_TICK) == fp32
    for name, row, flight in _cases():
        B, P = CE.tick_inputs(row, total_mass, flight)
        e = V.f32_tick_errors(oracle, B, P, _obs_state(oracle, B, "f64", row[2]))
        print("%-22s fp32 oracle against fp64 oracle: %s%s" % (name, "  ".join("%s %.2g" % kv for kv in e.items()),
                                                               "   (gates tau %.2g f %.2g)" % tuple(V.f32_gate(F32_TOL, x) for x in CE.F32_TICK[name]) if name in fp32 else ""))
        assert e["flips"] == 0, name
        for k, const in zip(("tau", "f"), CE.F32_TICK.get(name, ())):
            assert e[k] <= const <= 2 * e[k], (name, k, e[k], const)
        assert all(e[k] < F32_DYN / 4 for k in ("M", "h", "Jc", "pf")), (name, e)
        if "r" in e:
            assert e["integ"] < F32_OBS[0] / 4 and e["r"] < F32_OBS[1] / 4, (name, e)


def test_f32_rollout_constants_and_the_flight_rollouts(oracle, total_mass):
    """contact_edges.F32_ROLLOUT, likewise (status 0 on every tick of every rollout in both scalar types: asserted inside); and the rollouts with every
    robot in flight for the whole horizon end with status 0 and finite states"""
    w = CE.f32_rollout_errors(oracle, total_mass)
    print("rollouts: fp32 oracle against fp64 oracle: %s" % "  ".join("%s %.2g" % kv for kv in w.items()))
    for k, x in w.items():
        assert x <= CE.F32_ROLLOUT[k] <= 2 * x, (k, x)
    print("   gates: " + "  ".join("%s %.2g" % (k, V.f32_gate(g, CE.F32_ROLLOUT[k])) for k, g in
                                   (("q", F32_DYN), ("v", F32_DYN), ("tau_traj", F32_TOL), ("integ", F32_OBS[0]), ("r", F32_OBS[1]))))
    for n in (17, 66):
        for obs in (0, 1):
            B, P = CE.rollout_case(n, total_mass, obs, flight="all")
            o = V.oracle_rollout(oracle, B, P, 8, np.float64)
            assert np.all(o["status"] == 0) and np.all(np.isfinite(o["q"])) and np.all(np.isfinite(o["v"]))


def test_limit_cases_meet_their_conditions(oracle, total_mass):
    """The torque-limit cases of the GPU file: every re-solved QP has qp_status 0, at least 30 re-solved states have a steep stance foot, states within
    the limits occur too, none is clipped; fp64: every margin above the band of tests/util.py's _compare; fp32: at most 2 % of a case within it"""
    for n in CE.LIMIT_SIZES:
        for lim in CE.LIMITS:
            for dtype, obs in CE.LIMIT_MODES:
                B, P, integ, r = CE.limit_case(oracle, total_mass, n, lim, dtype, obs)
                ref = limit_ref.step_limited(oracle, P, B, lim, np.float64 if dtype == "f64" else np.float32, integ, r)
                one = ref["limited"] == 1
                steep = (CE.steep_feet(B["normals"]) & CE.stance(B["mask"])).any(axis=1)
                inside = ref["margin"] < CE.limit_band(dtype, lim)
                print("limit %g n=%-3d %s observer %d: %s re-solved, %d of them with a steep stance foot; smallest margin %.3g, %d states within the band"
                      % (lim, n, dtype, obs, np.bincount(ref["limited"], minlength=3), int((one & steep).sum()), ref["margin"].min(), int(inside.sum())))
                assert np.all(ref["qp_status"][one] == 0) and not (ref["limited"] == 2).any() and np.all(ref["status"] == 0)
                assert (one & steep).sum() >= 30 and (ref["limited"] == 0).sum() >= 10
                assert inside.mean() <= (0.0 if dtype == "f64" else CE.LIMIT_SKIP_CAP), (lim, n, dtype, obs, inside.mean())
