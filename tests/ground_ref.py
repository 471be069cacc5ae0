"""Ground-contact plant (wbc_ground_force_batch, wbc_integrate_ground_batch; include/wbc_hip.h "Ground-contact plant") restated in numpy, for the tests
(test infrastructure).

Row-per-state arrays in the dtype of q, like tests/gait_ref.py, so that the same code evaluated in float32 measures what single precision costs:
q [N, 19], v [N, 18], Jc [N, 216] (12 x 18 row-major), normals [N, 12], height [N, 4], mu [N, 4]; `legs` = limit_ref.leg_joints(flat), the caller's
joint indices of every foot's leg.
  ground_force       the law: dict(f_gr [N, 12], contact [N], gap [N, 4]) + the intermediate numbers the margins are stated on
  integrate_ground   the law, then the plant step with f = f_gr (float64: tests/envelope.py::integrate_ref)
  branch_case        a batch on which every foot takes every branch of the law, with every decision away from its switching point
  settle             the standing robot released 5 mm above flat ground: how the default parameters were fixed
  walk_case / closed_loop / cpu_walk   gait_ref's walking loop on the ground plant, last tick's contact fed to the gait, bumps under some feet
"""
import numpy as np

from oracle import oracle_py
from tests import envelope, gait_ref as GR, limit_ref, swing_ref as SR, walk_ref
from tests.util import unpack_M
from wbc_quadruped_dob_amd import synth

# wbc_ground_params_default.  Fixed with settle() below at synth.default_params' dt = 1e-3 (tests/test_ground_oracle.py holds the measured figures).
# The starting point k_n 2e4, c_n 200, c_t 500 did NOT settle: the four feet are coupled through the trunk, and the largest eigenvalue of
# dt (Jc M^-1 Jc^T) diag(c_t, c_t, c_n) over all twelve foot rows was 2.03 in the standing posture, past the explicit limit of 2 -- the foot forces
# alternated from tick to tick between 222 and 273 N for good, although every per-foot ratio c_n dt / m_eff is only 0.6.  c_n 150, c_t 200 bring that
# eigenvalue to 0.97 (stability_coupled).
DEFAULT_PARAMS = dict(k_n=2e4, c_n=150.0, c_t=200.0, f_touch=5.0)
PARITY_SIZES = (1, 15, 16, 17, 33)
MARGIN = 1e-3          # relative decision margins of branch_case
GAP_MARGIN = 1e-4      # m


def params(**kw):
    P = dict(DEFAULT_PARAMS)
    for k, val in kw.items():
        assert k in P, k
        P[k] = float(val)
    return P


_ORACLES = {}


def _oracle(flat):
    if id(flat) not in _ORACLES:
        _ORACLES[id(flat)] = oracle_py.Oracle(flat)
    return _ORACLES[id(flat)]


def foot_words(Jc, v, k, legs):
    """what a lane reads of Jc and v for foot k: lever [N, 3] (from the base-angular block -[d]x of the foot's rows), J_leg [N, 3, 3], qdot_leg [N, 3]"""
    J = Jc.reshape(Jc.shape[0], 12, 18)
    lever = np.stack([J[:, 3 * k + 1, 5], J[:, 3 * k + 2, 3], J[:, 3 * k + 0, 4]], 1)
    cols = [6 + j for j in legs[k]]
    return lever, J[:, 3 * k:3 * k + 3, cols], v[:, cols]


def ground_force(P, q, v, Jc, normals, height, mu, legs):
    """-> dict(f_gr, contact (int32), gap, raw [N, 4], fn [N, 4], gnorm [N, 4], cone [N, 4], vt [N, 4, 3]); arithmetic in q's dtype"""
    dt = q.dtype
    t = dt.type
    v, Jc, normals, height, mu = (np.asarray(a, dt) for a in (v, Jc, normals, height, mu))
    N = q.shape[0]
    out = dict(f_gr=np.zeros((N, 12), dt), contact=np.zeros(N, np.int32), gap=np.zeros((N, 4), dt), raw=np.zeros((N, 4), dt), fn=np.zeros((N, 4), dt),
               gnorm=np.zeros((N, 4), dt), cone=np.zeros((N, 4), dt), vt=np.zeros((N, 4, 3), dt))
    kn, cn, ct, ftouch = t(P["k_n"]), t(P["c_n"]), t(P["c_t"]), t(P["f_touch"])
    for k in range(4):
        lever, Jl, qd = foot_words(Jc, v, k, legs)
        n = normals[:, 3 * k:3 * k + 3]
        pf = q[:, 0:3] + lever
        vf = (v[:, 0:3] + np.cross(v[:, 3:6], lever).astype(dt) + np.einsum("nij,nj->ni", Jl, qd)).astype(dt)
        phi = (n * pf).sum(1) - height[:, k]
        vn = (n * vf).sum(1)
        vt = vf - vn[:, None] * n
        raw = -kn * phi - cn * vn
        fn = np.where((phi < 0) & (raw > 0), raw, t(0)).astype(dt)
        g = -ct * vt
        gn = np.sqrt((g * g).sum(1))
        cone = mu[:, k] * fn
        s = np.where(gn > cone, cone / np.where(gn > 0, gn, t(1)), t(1)).astype(dt)
        out["f_gr"][:, 3 * k:3 * k + 3] = fn[:, None] * n + s[:, None] * g
        out["contact"] |= (fn > ftouch).astype(np.int32) << k
        out["gap"][:, k], out["raw"][:, k], out["fn"][:, k], out["gnorm"][:, k], out["cone"][:, k], out["vt"][:, k] = phi, raw, fn, gn, cone, vt
    return out


def plant_step(dt_ctl, M, h, Jc, tau, f, tau_ext, q, v):
    """envelope.integrate_ref in the dtype of q (M unpacked [N, nv, nv]): what float32 costs is measured with this one; in float64 the two agree
    (tests/test_ground_oracle.py)"""
    dt = q.dtype
    t = dt.type
    M, h, Jc, tau, f, tau_ext, v = (np.asarray(a, dt) for a in (M, h, Jc, tau, f, tau_ext, v))
    N, nv = v.shape
    rhs = tau_ext - h + np.einsum("nij,ni->nj", Jc.reshape(N, -1, nv), f)
    rhs[:, 6:] += tau
    vn = (v + t(dt_ctl) * np.linalg.solve(M, rhs[:, :, None])[:, :, 0]).astype(dt)
    qn = q.copy()
    qn[:, 0:3] = q[:, 0:3] + t(dt_ctl) * vn[:, 0:3]
    w = vn[:, 3:6] * t(dt_ctl)
    th = np.sqrt((w * w).sum(1))
    big = th > t(1e-8)
    sc = np.where(big, np.sin(th / 2) / np.where(big, th, t(1)), t(0.5) - th * th / t(48)).astype(dt)
    cw = np.where(big, np.cos(th / 2), t(1) - th * th / t(8)).astype(dt)
    dx, dy, dz = (sc[:, None] * w).T
    x, y, z, ww = (q[:, 3:7] / np.sqrt((q[:, 3:7] ** 2).sum(1))[:, None]).T
    qn[:, 3:7] = np.stack([cw * x + dx * ww + dy * z - dz * y, cw * y - dx * z + dy * ww + dz * x, cw * z + dx * y - dy * x + dz * ww,
                           cw * ww - dx * x - dy * y - dz * z], 1)
    qn[:, 7:] = q[:, 7:] + t(dt_ctl) * vn[:, 6:]
    return qn.astype(dt), vn


def integrate_ground(P, dt_ctl, dyn, tau, normals, height, mu, tau_ext, q, v, legs):
    """-> (q', v', ground_force's dict); dyn = dict(M packed [N, 171], h, Jc) of the same tick; the arguments are not modified.  float64: the plant step is
    tests/envelope.py::integrate_ref with f = f_gr; float32: plant_step"""
    g = ground_force(P, q, v, dyn["Jc"], normals, height, mu, legs)
    tau_ext = np.zeros_like(v) if tau_ext is None else tau_ext
    M = unpack_M(np.asarray(dyn["M"], q.dtype))
    step = envelope.integrate_ref if q.dtype == np.float64 else plant_step
    qn, vn = step(dt_ctl, M, dyn["h"], dyn["Jc"], tau, g["f_gr"], tau_ext, q, v)
    return qn, vn, g


# ---- the branch case
# per-foot kinds: (gap as a function of the parameters, v_n, |g| / (mu f_n) or None for v_t = 0.3 m/s)
#   0 above the ground          1 penetrating but leaving fast: raw f_n < 0, clamped      2 sticking      3 sliding
#   4 sticking, f_n below f_touch (bit clear with f_n > 0)          5 sliding, f_n just above f_touch
NKINDS = 6
REST_EVERY = 15        # state i with i % 15 == 14 is the robot at rest but for pdot_z, n = e_z: v_t = 0 exactly on every foot


def _kind(P, kind):
    kn, ft = P["k_n"], P["f_touch"]
    return {0: (2e-3, 0.0, None), 1: (-1e-3, 0.5, None), 2: (-100.0 / kn, -0.05, 0.5), 3: (-60.0 / kn, 0.02, 3.0),
            4: (-0.6 * ft / kn, 0.0, 0.4), 5: (-1.4 * ft / kn, 0.0, 2.5)}[kind]


def branch_case(flat, total_mass, n, rank=0, P=None, states=None):
    """synth.make_batch(4, ...) states (tilted normals, three friction coefficients; states: a batch of make_batch's keys with unit normals, taken
    instead of drawing one -- tests/walk_edges.py); per foot the leg's joint velocities are solved for so that the foot
    has a chosen velocity, and `height` is placed so that it has a chosen gap: foot k of state i is of kind (i + 2 k) mod 6, and every 15th state
    (i mod 15 == 14) is a robot at rest but for pdot_z = -0.1 with n = e_z under every foot 5 mm in the ground -- v_f has one component, along n, so
    v_t = 0 exactly.  dict(q, v, normals, height, mu, dyn (M, h, Jc of the oracle), tau, tau_ext, kinds [n, 4] (-1 = the rest states))"""
    P = P or params()
    orc = _oracle(flat)
    legs = limit_ref.leg_joints(flat)
    B = synth.make_batch(4, n, total_mass, rank=110 + rank) if states is None else states
    rng = np.random.default_rng(synth.SEED + 1300 + rank)
    q, v, normals, mu = B["q"], B["v"].copy(), B["normals"].copy(), B["mu"]
    assert q.shape[0] == n
    rest = np.arange(n) % REST_EVERY == REST_EVERY - 1
    v[rest] = 0.0
    v[rest, 2] = -0.1
    normals[rest] = np.tile([0.0, 0.0, 1.0], 4)
    Jc = orc.dynamics(q, v)["Jc"]            # (a function of q alone)
    kinds = np.where(rest[:, None], -1, (np.arange(n)[:, None] + 2 * np.arange(4)[None, :]) % NKINDS)
    height = np.zeros((n, 4))
    for k in range(4):
        lever, Jl, _ = foot_words(Jc, v, k, legs)
        nk = normals[:, 3 * k:3 * k + 3]
        tang = rng.normal(size=(n, 3))
        tang -= (tang * nk).sum(1)[:, None] * nk
        tang /= np.linalg.norm(tang, axis=1, keepdims=True)
        gap = np.full(n, -5e-3)
        for i in np.nonzero(~rest)[0]:
            gap[i], vn, ratio = _kind(P, kinds[i, k])
            fn = max(0.0, -P["k_n"] * gap[i] - P["c_n"] * vn) if gap[i] < 0 else 0.0
            vt = 0.3 if ratio is None else ratio * mu[i, k] * fn / P["c_t"]
            vf = vn * nk[i] + vt * tang[i]
            v[i, [6 + j for j in legs[k]]] = np.linalg.solve(Jl[i], vf - v[i, 0:3] - np.cross(v[i, 3:6], lever[i]))
        height[:, k] = (nk * (q[:, 0:3] + lever)).sum(1) - gap
    dyn = orc.dynamics(q, v)
    tau = rng.uniform(-20, 20, (n, 12))
    tau_ext = np.zeros((n, 18)); tau_ext[:, 0:3] = B["push"]
    return dict(q=q, v=v, normals=normals, height=height, mu=mu, dyn={k: dyn[k] for k in ("M", "h", "Jc")}, tau=tau, tau_ext=tau_ext, kinds=kinds)


def branches_taken(P, g):
    """set of (foot, branch) of a ground_force result, evaluated on its own numbers: 0 gap >= 0; 1 penetrating, raw f_n <= 0 (clamped); 2 sticking
    (0 < |g| <= mu f_n); 3 sliding (|g| > mu f_n > 0); 4 v_t = 0 exactly with f_n > 0; 5 contact bit set; 6 bit clear with f_n > 0"""
    seen = set()
    for k in range(4):
        phi, raw, fn, gn, cone = (g[x][:, k] for x in ("gap", "raw", "fn", "gnorm", "cone"))
        bit = ((g["contact"] >> k) & 1) == 1
        vt0 = np.all(g["vt"][:, k] == 0, axis=1)
        for b, m in enumerate((phi >= 0, (phi < 0) & (raw <= 0), (fn > 0) & (gn > 0) & (gn <= cone), (fn > 0) & (gn > cone), vt0 & (fn > 0), bit,
                               ~bit & (fn > 0))):
            if m.any():
                seen.add((k, b))
    return seen


ALL_BRANCHES = {(k, b) for k in range(4) for b in range(7)}


def margins(P, g):
    """the four decision margins of a ground_force result, each as (smallest value found) / (what the case must keep): all >= 1 passes"""
    fmax = float(g["fn"].max()) if g["fn"].max() > 0 else 1.0
    cone, gn = g["cone"], g["gnorm"]
    on = cone > 0
    return dict(gap=float(np.abs(g["gap"]).min() / GAP_MARGIN),
                touch=float(np.abs(g["fn"] - P["f_touch"]).min() / (MARGIN * fmax)),
                cone=float((np.abs(gn - cone)[on] / (MARGIN * cone[on])).min()) if on.any() else np.inf,
                raw=float(np.abs(g["raw"]).min() / (MARGIN * fmax)))


# ground_force / integrate_ground in float32 against float64 on branch_case(n, rank=n) of PARITY_SIZES (synthetic model, default parameters, dt 1e-3),
# largest error relative to the largest entry of the array, rounded up to two digits: what single precision costs.  tests/test_ground_oracle.py checks
# the numbers, tests/test_gpu_ground.py gates the device's fp32 results at 8 x them.
F32_ERR = dict(f_gr=1.1e-5, gap=1.3e-5, q=6.5e-8, v=3.7e-7)


def f32_errors(flat, total_mass, dt_ctl=1e-3):
    """the measurement behind F32_ERR; asserts on the way that float32 takes the same branches (contact words equal)"""
    P = params()
    legs = limit_ref.leg_joints(flat)
    worst = dict(f_gr=0.0, gap=0.0, q=0.0, v=0.0)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    for n in PARITY_SIZES:
        c = branch_case(flat, total_mass, n, rank=n, P=P)
        q64, v64, g64 = integrate_ground(P, dt_ctl, c["dyn"], c["tau"], c["normals"], c["height"], c["mu"], c["tau_ext"], c["q"], c["v"], legs)
        d32 = {k: f(x) for k, x in c["dyn"].items()}
        q32, v32, g32 = integrate_ground(P, dt_ctl, d32, f(c["tau"]), f(c["normals"]), f(c["height"]), f(c["mu"]), f(c["tau_ext"]), f(c["q"]),
                                         f(c["v"]), legs)
        assert np.array_equal(g32["contact"], g64["contact"])
        for what, a, b in (("f_gr", g32["f_gr"], g64["f_gr"]), ("gap", g32["gap"], g64["gap"]), ("q", q32, q64), ("v", v32, v64)):
            worst[what] = max(worst[what], float(np.abs(a - b).max() / np.abs(b).max()))
    return worst


# ---- how the defaults were fixed: a standing robot released 5 mm above flat ground
SETTLE_DROP, SETTLE_TICKS, SETTLE_TOL = 5e-3, 1500, 1e-3


def stand_case(flat, oracle, n=1):
    """swing_ref.loop_case's standing robots, all feet in stance, flat ground SETTLE_DROP below the lowest foot.  dict(q, v, plan, normals, mu, mask, height)"""
    c = SR.loop_case(flat, oracle, n)
    c["mask"] = np.full(n, 0b1111, np.int32)
    pfz = np.stack([SR.foot_kin(flat, k, c["q"], c["v"])["pf"][:, 2] for k in range(4)], 1)
    c["height"] = np.repeat(pfz.min(1, keepdims=True) - SETTLE_DROP, 4, 1)
    return c


def stability_ratios(P, dt_ctl, dyn, normals):
    """per foot of every state: (c_n dt / m_eff, k_n dt^2 / m_eff), m_eff = 1 / (n Jc_k M^-1 Jc_k^T n).  [N, 4] each"""
    M = unpack_M(np.asarray(dyn["M"], np.float64))
    N = M.shape[0]
    J = np.asarray(dyn["Jc"], np.float64).reshape(N, 12, 18)
    a, b = np.zeros((N, 4)), np.zeros((N, 4))
    for k in range(4):
        row = np.einsum("ni,nij->nj", normals[:, 3 * k:3 * k + 3], J[:, 3 * k:3 * k + 3])
        inv_m = np.einsum("ni,ni->n", row, np.linalg.solve(M, row[:, :, None])[:, :, 0])
        a[:, k], b[:, k] = P["c_n"] * dt_ctl * inv_m, P["k_n"] * dt_ctl ** 2 * inv_m
    return a, b


def stability_coupled(P, dt_ctl, dyn):
    """[N]: the largest eigenvalue of dt (Jc M^-1 Jc^T) D, D = diag(c_t, c_t, c_n) per foot (flat ground, n = e_z): the explicit damping term is
    stable below 2"""
    M = unpack_M(np.asarray(dyn["M"], np.float64))
    J = np.asarray(dyn["Jc"], np.float64).reshape(M.shape[0], 12, 18)
    D = np.kron(np.eye(4), np.diag([P["c_t"], P["c_t"], P["c_n"]]))
    return np.array([np.linalg.eigvals(dt_ctl * (J[s] @ np.linalg.solve(M[s], J[s].T)) @ D).real.max() for s in range(M.shape[0])])


def settle(flat, oracle, P=None, ticks=SETTLE_TICKS, n=1):
    """The standing loop oracle.reference -> oracle.step (all feet planned in stance) -> integrate_ground.  Returns dict(weight: sum_k n . f_gr,k per
    tick [ticks, n], pen: mean penetration per tick, contact [ticks, n], settle_tick: the first tick from which the weight stays within SETTLE_TOL of
    m g to the end (None: never), m_g, ratios: stability_ratios at the end, status_ok)"""
    P = P or params()
    prm, G = synth.default_params(observer_order=0), SR.loop_ref_params()
    legs = limit_ref.leg_joints(flat)
    c = stand_case(flat, oracle, n)
    q, v = c["q"].copy(), c["v"].copy()
    weight, pen, contact, ok = [], [], [], True
    for k in range(ticks):
        ref = oracle.reference(G, q, v, c["plan"], 0.0)
        tick = oracle.step(prm, q, v, ref["w_des"], ref["vdot_des"], c["normals"], c["mu"], c["mask"])
        ok = ok and bool(np.all(tick["status"] == 0))
        dyn = oracle.dynamics(q, v)
        q, v, g = integrate_ground(P, prm["dt"], dyn, tick["tau"], c["normals"], c["height"], c["mu"], None, q, v, legs)
        weight.append(g["fn"].sum(1)); pen.append(-g["gap"].mean(1)); contact.append(g["contact"])
    weight, pen, contact = np.array(weight), np.array(pen), np.array(contact)
    m_g = float(np.sum(flat["mass"])) * float(np.linalg.norm(flat["gravity"]))
    return dict(weight=weight, pen=pen, contact=contact, status_ok=ok, q=q, v=v, ratios=stability_ratios(P, prm["dt"], dyn, c["normals"]),
                coupled=stability_coupled(P, prm["dt"], dyn), m_g=m_g)


def settle_tick(weight, m_g, tol=SETTLE_TOL):
    """first tick from which |weight - m g| <= tol m g holds to the end, for every robot; None if the last tick is outside"""
    bad = np.nonzero(np.any(np.abs(weight - m_g) > tol * m_g, axis=1))[0]
    if len(bad) == 0:
        return 0
    return None if bad[-1] == len(weight) - 1 else int(bad[-1] + 1)


# ---- the walking loop on the ground plant
BUMP, BUMP_TICK = 0.015, 64     # m; the tick at which the terrain under the marked feet changes: feet 1 and 2 lift at tick 0 and are at the apex of their
                                # first swing (5 cm up) at tick 64 of its 128, so the new ground is met on the way down, as a walking robot meets it
WALK_TICKS = GR.WALK_TICKS


def walk_case(flat, oracle, n):
    """gait_ref.walk_case on the ground: height0 [n, 4] = every foot's own starting height (zero gap at the start), height1 = height0 with a bump of
    +BUMP under foot 1 of the even robots and a hole of -BUMP under foot 2 of the robots with index 4 j + 1; the loop switches at BUMP_TICK."""
    c = GR.walk_case(flat, oracle, n)
    pfz = np.stack([SR.foot_kin(flat, k, c["q"], c["v"])["pf"][:, 2] for k in range(4)], 1)
    c["height0"] = pfz.copy()
    c["height1"] = pfz.copy()
    idx = np.arange(n)
    c["height1"][idx % 2 == 0, 1] += BUMP
    c["height1"][idx % 4 == 1, 2] -= BUMP
    return c


def early_touchdowns(GP, phases, events):
    """[(tick, state, foot, u)] of every touchdown event that fell inside the foot's swing window (u < 1), from the phases the gait calls left
    ([ticks, N], exact dyadic numbers in the walking loop) and their events"""
    out = []
    for f in range(4):
        pk = (phases + GP["offset"][f]) % 1.0
        for k, s in zip(*np.nonzero(((events >> (4 + f)) & 1) & (pk >= GP["duty"][f]))):
            out.append((int(k), int(s), f, float((pk[k, s] - GP["duty"][f]) / (1.0 - GP["duty"][f]))))
    return sorted(out)


def closed_loop(flat, oracle, case, ticks=WALK_TICKS, P=None, sensed=True, q0=None):
    """gait(contact = last tick's, or None when not sensed) -> oracle.reference -> swing_reference -> oracle.step -> integrate_ground, per tick.
    Returns dict(q, v at the end; masks, events, contacts [ticks, N]; status_ok; touch_margin: the smallest |f_n - f_touch| / max f_n over all feet and
    ticks; early: list of (tick, state, foot, u) of every touchdown event with u < 1, u the foot's place in its swing window)"""
    P = P or params()
    GP, fns = GR.walk_params(flat), []
    w = walk_ref.closed_loop(flat, oracle, case, ticks, walk_ref.ground_plant(flat, case, P), GR.WALK_SWING_PARAMS, gait=GP,
                             sensed="plant" if sensed else None, q0=q0, extras=lambda now: fns.append(now["ground"]["fn"]))
    fns = np.array(fns)
    return dict(q=w["q"], v=w["v"], masks=w["masks"], events=w["events"], contacts=w["contacts"], status_ok=w["status_ok"],
                early=early_touchdowns(GP, w["phases"], w["events"]),
                touch_margin=float(np.abs(fns - P["f_touch"]).min() / fns.max()), fn_max=float(fns.max()))


def cpu_walk(flat, oracle, n):
    """(case, closed_loop(case)) of n robots, computed once per process and shared by the tests that need it: read only"""
    return walk_ref.cached(("ground", id(flat), n), lambda: walk_case(flat, oracle, n), lambda case: closed_loop(flat, oracle, case))


# amplification of a 1e-12 relative perturbation of q0 over the walking loop, measured by tests/test_ground_oracle.py (2.3), rounded up: the device loop's
# gate in tests/test_gpu_ground.py is max(1e-6, 10 A 1e-9) with 1e-9 the per-tick device error DESIGN.md 6 reports
WALK_AMPLIFICATION = 5.0
