"""Stiction on the ground plant (wbc_ground_stick_force_batch, wbc_integrate_ground_stick_batch; include/wbc_hip.h "Stiction on the ground plant")
restated in numpy, for the tests (test infrastructure).  The law is ground_ref's with a per-foot anchor spring in the tangential force.

Row-per-state arrays in the dtype of q like tests/ground_ref.py, plus anchor [N, 12] (rows 3k .. 3k+2 of the device buffer = columns here) and
stick [N] int32.  The arguments are never modified: the new anchor and stick word come back in the result.
  stick_force              the law: ground_force's dict + anchor, stick (new), pf, ft, e, loaded, slid, had
  integrate_ground_stick   the law, then the plant step with f = f_gr
  branch_case              ground_ref.branch_case with anchors and stick words such that every foot takes every branch of the law
  stand_loop               the standing robot on tilted planes (slope hold, slide, flat settle): how the default k_t was fixed
  walk_case / closed_loop / cpu_walk   ground_ref's walking loop on the plant with stiction, starting at the equilibrium penetration
"""
import numpy as np

from tests import gait_ref as GR, ground_ref as R, limit_ref, swing_ref as SR, walk_ref
from tests.util import unpack_M
from wbc_quadruped_dob_amd import synth

# wbc_stiction_params_default.  Fixed with stand_loop / closed_loop below (tests/test_stick_oracle.py holds the measured figures): the starting point
# k_t = k_n = 2e4 passed the slope, the slide, the flat settle and the walking loop at dt = 1e-3 and 2^-10, so it was kept.
DEFAULT_KT = 2e4
PARITY_SIZES = R.PARITY_SIZES


def stick_force(P, k_t, q, v, Jc, normals, height, mu, anchor, stick, legs):
    """-> ground_force's dict (f_gr, contact, gap, raw, fn, gnorm (|g| with the spring term), cone, vt) + anchor [N, 12] and stick [N] int32 (new),
    pf [N, 4, 3], ft [N, 4, 3], e [N, 4, 3], loaded, slid, had [N, 4] bool; arithmetic in q's dtype"""
    dt = q.dtype
    t = dt.type
    v, Jc, normals, height, mu, anchor = (np.asarray(a, dt) for a in (v, Jc, normals, height, mu, anchor))
    stick = np.asarray(stick, np.int32)
    N = q.shape[0]
    z = lambda *s: np.zeros((N,) + s, dt)
    out = dict(f_gr=z(12), contact=np.zeros(N, np.int32), gap=z(4), raw=z(4), fn=z(4), gnorm=z(4), cone=z(4), vt=z(4, 3), anchor=anchor.copy(),
               stick=np.zeros(N, np.int32), pf=z(4, 3), ft=z(4, 3), e=z(4, 3), loaded=np.zeros((N, 4), bool), slid=np.zeros((N, 4), bool),
               had=np.zeros((N, 4), bool))
    kn, cn, ct, ftouch, kt = t(P["k_n"]), t(P["c_n"]), t(P["c_t"]), t(P["f_touch"]), t(k_t)
    for k in range(4):
        # (ground_ref.ground_force's lines down to f_n)
        lever, Jl, qd = R.foot_words(Jc, v, k, legs)
        n = normals[:, 3 * k:3 * k + 3]
        pf = q[:, 0:3] + lever
        vf = (v[:, 0:3] + np.cross(v[:, 3:6], lever).astype(dt) + np.einsum("nij,nj->ni", Jl, qd)).astype(dt)
        phi = (n * pf).sum(1) - height[:, k]
        vn = (n * vf).sum(1)
        vt = vf - vn[:, None] * n
        raw = -kn * phi - cn * vn
        fn = np.where((phi < 0) & (raw > 0), raw, t(0)).astype(dt)
        # the anchor spring
        had = ((stick >> k) & 1) == 1
        loaded = fn > 0
        use = had & loaded
        a = np.where(use[:, None], anchor[:, 3 * k:3 * k + 3], pf)
        da = pf - a
        e = da - (n * da).sum(1)[:, None] * n
        g = -kt * e - ct * vt
        gn = np.sqrt((g * g).sum(1))
        cone = mu[:, k] * fn
        over = gn > cone
        s = np.where(over, cone / np.where(gn > 0, gn, t(1)), t(1)).astype(dt)
        ft = s[:, None] * g
        slid = loaded & over
        move = loaded & (over | ~had)
        anew = np.where(slid[:, None], pf - s[:, None] * e, pf)
        out["anchor"][:, 3 * k:3 * k + 3] = np.where(move[:, None], anew, anchor[:, 3 * k:3 * k + 3])
        out["stick"] |= (loaded.astype(np.int32) << k) | (slid.astype(np.int32) << (4 + k))
        out["f_gr"][:, 3 * k:3 * k + 3] = fn[:, None] * n + ft
        out["contact"] |= (fn > ftouch).astype(np.int32) << k
        for key, val in (("gap", phi), ("raw", raw), ("fn", fn), ("gnorm", gn), ("cone", cone), ("vt", vt), ("pf", pf), ("ft", ft), ("e", e),
                         ("loaded", loaded), ("slid", slid), ("had", had)):
            out[key][:, k] = val
    return out


def integrate_ground_stick(P, k_t, dt_ctl, dyn, tau, normals, height, mu, tau_ext, q, v, anchor, stick, legs):
    """-> (q', v', stick_force's dict); dyn = dict(M packed [N, 171], h, Jc) of the same tick.  The plant step is ground_ref.integrate_ground's"""
    g = stick_force(P, k_t, q, v, dyn["Jc"], normals, height, mu, anchor, stick, legs)
    tau_ext = np.zeros_like(v) if tau_ext is None else tau_ext
    M = unpack_M(np.asarray(dyn["M"], q.dtype))
    step = R.envelope.integrate_ref if q.dtype == np.float64 else R.plant_step
    qn, vn = step(dt_ctl, M, dyn["h"], dyn["Jc"], tau, g["f_gr"], tau_ext, q, v)
    return qn, vn, g


# ---- the branch case
# ground_ref.branch_case decides gap, v_n and |c_t v_t| / (mu f_n) per foot (kind (i + 2 k) mod 6 of foot k of state i).  Added here:
#   in bit k of state i = (i // 6) mod 2 (the rest states: set), so that with n >= 15 every kind of every foot comes with the bit clear and set;
#   bits 4 ... of every odd state's word hold junk (only bits 0-3 are read)
#   a foot with its bit set gets an anchor with the stretch e = SPRING (c_t |v_t| / k_t) (cos TH t + sin TH n x t), t = v_t / |v_t|, plus 3 mm along n
#     (the law projects it out): |g| = 1.51 x the viscous term, so kinds 2, 4 stick at 0.75, 0.60 of the cone and kinds 3, 5 slide at 4.5, 3.8
#   a rest state (v_t = 0 exactly) gets e of REST_RATIO[j] mu f_n / k_t, j = its index among the rest states: the first sticks, the second slides
#   every other anchor word is junk the law must not look at (unloaded feet: untouched; first loaded tick: replaced by p_f)
SPRING, TH = 0.6, 0.7
REST_RATIO = (0.5, 2.0)
JUNK = 7.25


def branch_case(flat, total_mass, n, rank=0, P=None, k_t=DEFAULT_KT, states=None):
    """ground_ref.branch_case (states: handed through) + anchor [n, 12], stick [n] int32"""
    P = P or R.params()
    legs = limit_ref.leg_joints(flat)
    c = R.branch_case(flat, total_mass, n, rank=rank, P=P, states=states)
    g = R.ground_force(P, c["q"], c["v"], c["dyn"]["Jc"], c["normals"], c["height"], c["mu"], legs)
    rng = np.random.default_rng(synth.SEED + 1400 + rank)
    rest = c["kinds"][:, 0] == -1
    bit = np.where(rest, 1, (np.arange(n) // 6) % 2).astype(np.int32)
    stick = bit * 0b1111 | np.where(np.arange(n) % 2 == 1, 0x7ab0, 0).astype(np.int32)
    anchor = JUNK + rng.uniform(-1, 1, (n, 12))
    nrest = 0
    for i in range(n):
        for k in range(4):
            if not bit[i] or g["fn"][i, k] == 0:
                continue
            nk = c["normals"][i, 3 * k:3 * k + 3]
            lever = R.foot_words(c["dyn"]["Jc"], c["v"], k, legs)[0][i]
            pf = c["q"][i, 0:3] + lever
            if rest[i]:
                th = 0.4 + k
                e = REST_RATIO[min(nrest, 1)] * g["cone"][i, k] / k_t * np.array([np.cos(th), np.sin(th), 0.0])     # n = e_z
            else:
                vt = g["vt"][i, k]
                tv = vt / np.linalg.norm(vt)
                e = SPRING * P["c_t"] * np.linalg.norm(vt) / k_t * (np.cos(TH) * tv + np.sin(TH) * np.cross(nk, tv))
            anchor[i, 3 * k:3 * k + 3] = pf - e - 3e-3 * nk
        nrest += int(rest[i])
    c.update(anchor=anchor, stick=stick)
    return c


def branches_taken(g):
    """set of (foot, branch) of a stick_force result, evaluated on its own numbers: 0 unloaded with the in bit set; 1 unloaded with it clear; 2 first
    loaded tick (bit clear, f_n > 0); 3 anchored and sticking; 4 anchored and sliding; 5 v_t = 0 exactly with e != 0 and f_n > 0; 6 contact bit set;
    7 contact bit clear with f_n > 0"""
    seen = set()
    for k in range(4):
        had, loaded, slid = g["had"][:, k], g["loaded"][:, k], g["slid"][:, k]
        bit = ((g["contact"] >> k) & 1) == 1
        vt0 = np.all(g["vt"][:, k] == 0, axis=1) & np.any(g["e"][:, k] != 0, axis=1)
        for b, m in enumerate((~loaded & had, ~loaded & ~had, loaded & ~had, loaded & had & ~slid, loaded & had & slid, vt0 & loaded, bit,
                               ~bit & loaded)):
            if m.any():
                seen.add((k, b))
    return seen


ALL_BRANCHES = {(k, b) for k in range(4) for b in range(8)}


def margins(P, g):
    """ground_ref.margins on a stick_force result: gap, raw, touch, and cone with the spring term in |g| (gnorm is the law's |g|)"""
    return R.margins(P, g)


# stick_force / integrate_ground_stick in float32 against float64 on branch_case(n, rank=n) of PARITY_SIZES (synthetic model, default parameters,
# dt 1e-3), largest error relative to the largest entry of the array (anchor: over the words the law wrote), rounded up to two digits.
# tests/test_stick_oracle.py checks the numbers, tests/test_gpu_stick.py gates the device's fp32 results at 8 x them.
F32_ERR = dict(f_gr=1.1e-5, gap=1.3e-5, anchor=6.9e-8, q=6.5e-8, v=5.4e-7)


def f32_errors(flat, total_mass, dt_ctl=1e-3):
    """the measurement behind F32_ERR; asserts on the way that float32 takes the same branches (stick and contact words equal)"""
    P = R.params()
    legs = limit_ref.leg_joints(flat)
    worst = dict(f_gr=0.0, gap=0.0, anchor=0.0, q=0.0, v=0.0)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    for n in PARITY_SIZES:
        c = branch_case(flat, total_mass, n, rank=n, P=P)
        q64, v64, g64 = integrate_ground_stick(P, DEFAULT_KT, dt_ctl, c["dyn"], c["tau"], c["normals"], c["height"], c["mu"], c["tau_ext"], c["q"],
                                               c["v"], c["anchor"], c["stick"], legs)
        d32 = {k: f(x) for k, x in c["dyn"].items()}
        q32, v32, g32 = integrate_ground_stick(P, DEFAULT_KT, dt_ctl, d32, f(c["tau"]), f(c["normals"]), f(c["height"]), f(c["mu"]), f(c["tau_ext"]),
                                               f(c["q"]), f(c["v"]), f(c["anchor"]), c["stick"], legs)
        assert np.array_equal(g32["contact"], g64["contact"]) and np.array_equal(g32["stick"], g64["stick"])
        w = written_anchor(g64, c["anchor"])
        assert np.array_equal(w, written_anchor(g32, f(c["anchor"])))
        pairs = [("f_gr", g32["f_gr"], g64["f_gr"]), ("gap", g32["gap"], g64["gap"]), ("q", q32, q64), ("v", v32, v64)]
        if w.any():
            pairs.append(("anchor", g32["anchor"][w], g64["anchor"][w]))
        for what, a, b in pairs:
            worst[what] = max(worst[what], float(np.abs(a - b).max() / np.abs(b).max()))
    return worst


def written_anchor(g, anchor_in):
    """[N, 12] bool: the anchor words the law moved (a loaded foot that slid or had no anchor); every other word equals the input bit for bit"""
    move = g["loaded"] & (g["slid"] | ~g["had"])
    assert np.array_equal(g["anchor"][~np.repeat(move, 3, 1)], np.asarray(anchor_in, g["anchor"].dtype)[~np.repeat(move, 3, 1)])
    return np.repeat(move, 3, 1)


# ---- how the default k_t was fixed: the standing robot on tilted planes
SLOPE, SLOPE_TICKS, SLOPE_FROM = 0.2, 1500, 500      # rad about y; the drift is measured over ticks SLOPE_FROM ... SLOPE_TICKS
SLIDE_MU, SLIDE_TICKS = 0.1, 150


def slope_case(flat, oracle, n=1, tilt=SLOPE):
    """ground_ref.stand_case with every foot on its own plane n = (sin tilt, 0, cos tilt), SETTLE_DROP under the foot"""
    c = R.stand_case(flat, oracle, n)
    nrm = np.array([np.sin(tilt), 0.0, np.cos(tilt)])
    c["normals"] = np.tile(nrm, (n, 4))
    pf = np.stack([SR.foot_kin(flat, k, c["q"], c["v"])["pf"] for k in range(4)], 1)      # [n, 4, 3]
    c["height"] = pf @ nrm - R.SETTLE_DROP
    c["downhill"] = np.array([np.cos(tilt), 0.0, -np.sin(tilt)])
    return c


def stability_spring(P, k_t, dt_ctl, dyn):
    """[N]: the largest eigenvalue of dt^2 (Jc M^-1 Jc^T) diag(k_t, k_t, k_n) per foot (flat ground, n = e_z): b of the rule b < 4 - 2 a for one mode of
    the semi-implicit step, a = ground_ref.stability_coupled"""
    M = unpack_M(np.asarray(dyn["M"], np.float64))
    J = np.asarray(dyn["Jc"], np.float64).reshape(M.shape[0], 12, 18)
    D = np.kron(np.eye(4), np.diag([k_t, k_t, P["k_n"]]))
    return np.array([np.linalg.eigvals(dt_ctl ** 2 * (J[s] @ np.linalg.solve(M[s], J[s].T)) @ D).real.max() for s in range(M.shape[0])])


def stand_loop(flat, oracle, case, k_t=DEFAULT_KT, ticks=SLOPE_TICKS, mu_plant=None, P=None):
    """The standing loop oracle.reference -> oracle.step (all feet planned in stance, the controller's mu = case["mu"]) -> integrate_ground_stick (the
    plant's mu = mu_plant or the controller's).  Returns per-tick records: pf [ticks, n, 4, 3] (the positions the law saw), f_gr, ft, e, fn, gap,
    stick, contact, status_ok [ticks]; q, v at the end; dyn of the last tick; m_g"""
    P = P or R.params()
    prm, G = synth.default_params(observer_order=0), SR.loop_ref_params()
    legs = limit_ref.leg_joints(flat)
    n = case["q"].shape[0]
    q, v = case["q"].copy(), case["v"].copy()
    mu_p = case["mu"] if mu_plant is None else np.full_like(case["mu"], mu_plant)
    anchor, stick = np.zeros((n, 12)), np.zeros(n, np.int32)
    rec = {k: [] for k in ("pf", "f_gr", "ft", "e", "fn", "gap", "stick", "contact", "status_ok")}
    for k in range(ticks):
        ref = oracle.reference(G, q, v, case["plan"], 0.0)
        tick = oracle.step(prm, q, v, ref["w_des"], ref["vdot_des"], case["normals"], case["mu"], case["mask"])
        dyn = oracle.dynamics(q, v)
        q, v, g = integrate_ground_stick(P, k_t, prm["dt"], dyn, tick["tau"], case["normals"], case["height"], mu_p, None, q, v, anchor, stick, legs)
        anchor, stick = g["anchor"], g["stick"]
        for key in ("pf", "f_gr", "ft", "e", "fn", "gap", "stick", "contact"):
            rec[key].append(g[key])
        rec["status_ok"].append(bool(np.all(tick["status"] == 0)))
    out = {k: np.array(x) for k, x in rec.items()}
    out.update(q=q, v=v, dyn=dyn, m_g=float(np.sum(flat["mass"])) * float(np.linalg.norm(flat["gravity"])), dt=prm["dt"])
    return out


def drift(rec, a=SLOPE_FROM, b=None):
    """[n, 3]: how far the mean of a robot's four feet moved between tick a and the last tick (b)"""
    b = len(rec["pf"]) - 1 if b is None else b
    return rec["pf"][b].mean(1) - rec["pf"][a].mean(1)


_STANDS = {}


def cpu_slope(flat, oracle, k_t):
    """(slope_case, stand_loop on it with k_t), one robot, computed once per process and shared: read only"""
    key = (id(flat), float(k_t))
    if key not in _STANDS:
        case = slope_case(flat, oracle, 1)
        _STANDS[key] = (case, stand_loop(flat, oracle, case, k_t))
    return _STANDS[key]


# ---- the walking loop on the plant with stiction
WALK_TICKS = R.WALK_TICKS
SLIP_LOAD = 50.0      # N: the slip path counts |v_t| dt of a foot in the ticks in which it carries more than this


def walk_case(flat, oracle, n, P=None):
    """ground_ref.walk_case with both height arrays raised by m g / (4 k_n): the feet start at the equilibrium penetration, so that no foot's first
    loaded tick is decided by rounding (at zero gap it is, and with an anchor the tick a foot loads decides where it sticks)"""
    P = P or R.params()
    c = R.walk_case(flat, oracle, n)
    up = float(np.sum(flat["mass"])) * float(np.linalg.norm(flat["gravity"])) / (4 * P["k_n"])
    c["height0"] = c["height0"] + up
    c["height1"] = c["height1"] + up
    return c


def closed_loop(flat, oracle, case, k_t=DEFAULT_KT, ticks=WALK_TICKS, P=None, q0=None):
    """ground_ref.closed_loop (sensed contact) with integrate_ground_stick as its last link.  Returns ground_ref.closed_loop's dict + sticks [ticks, N],
    slip: the tangential path sum |v_t| dt (m, per robot) of the feet over the ticks in which they carry more than SLIP_LOAD"""
    P = P or R.params()
    GP, sticks, fns, slips = GR.walk_params(flat), [], [], []

    def extras(now):
        g = now["ground"]
        sticks.append(g["stick"].copy()); fns.append(g["fn"])
        slips.append(float((np.linalg.norm(g["vt"], axis=2) * GR.DYADIC_DT)[g["fn"] > SLIP_LOAD].sum()))

    w = walk_ref.closed_loop(flat, oracle, case, ticks, walk_ref.ground_plant(flat, case, P, k_t), GR.WALK_SWING_PARAMS, gait=GP, sensed="plant",
                             q0=q0, extras=extras)
    fns = np.array(fns)
    return dict(q=w["q"], v=w["v"], masks=w["masks"], events=w["events"], contacts=w["contacts"], sticks=np.array(sticks), status_ok=w["status_ok"],
                early=R.early_touchdowns(GP, w["phases"], w["events"]), slip=sum(slips, 0.0) / case["q"].shape[0],
                touch_margin=float(np.abs(fns - P["f_touch"]).min() / fns.max()), fn_max=float(fns.max()))


def cpu_walk(flat, oracle, n, k_t=DEFAULT_KT):
    """(case, closed_loop(case, k_t)) of n robots, computed once per process and shared by the tests that need it: read only"""
    return walk_ref.cached(("stick", id(flat), n, float(k_t)), lambda: walk_case(flat, oracle, n), lambda case: closed_loop(flat, oracle, case, k_t))


# amplification of a 1e-12 relative perturbation of q0 over the walking loop with stiction, measured by tests/test_stick_oracle.py (2.9), rounded up: the
# device loop's gate in tests/test_gpu_stick.py is max(1e-6, 10 A 1e-9), the rule of tests/test_gpu_ground.py
WALK_AMPLIFICATION = 3.0
