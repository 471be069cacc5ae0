"""Base state from leg odometry (wbc_base_estimate_batch, include/wbc_hip.h "Base state from leg odometry") restated in numpy, for the tests (test
infrastructure).  Row-per-state arrays like everything in oracle_py, arithmetic in the dtype of q, so that the same code in float32 measures what
single precision costs.
  leg_terms       lever_k = R d_k and u_k = R vf_k of the four feet from swing_ref.foot_kin with the base at the origin and at rest
  estimate        the law, vectorised            estimate_loop   the same law state by state and foot by foot (pins the vectorised form)
  branch_case     inputs that take every branch per foot in every 16 states, junk in every word the law must not read
  f32_errors      the measurement behind F32_ERR
  closed_loop     the walking loop with the controller links on q_est, v_est and the plant on the truth (estimated = False: the same loop on the truth)
"""
import numpy as np

from tests import contact_ref, gait_ref as GR, ground_ref as GND, limit_ref, stick_ref, swing_ref as SR, walk_ref
from wbc_quadruped_dob_amd import synth

DEFAULT_PARAMS = dict(a_v=0.125, a_p=0.25)      # wbc_odom_params_default
PARITY_SIZES = (1, 15, 16, 17, 33, 64)


def params(**kw):
    P = dict(DEFAULT_PARAMS)
    assert set(kw) <= set(P), kw
    P.update(kw)
    return P


def leg_terms(flat, q, v):
    """-> lever [N, 4, 3], u [N, 4, 3] in q's dtype.  Rows 0-2 of q and v are not read (they are replaced by zeros before foot_kin sees them)."""
    q0, v0 = np.array(q), np.array(v, q.dtype)
    q0[:, 0:3] = 0
    v0[:, 0:3] = 0
    K = [SR.foot_kin(flat, k, q0, v0) for k in range(4)]
    return np.stack([x["d"] for x in K], 1), np.stack([x["Jv"] for x in K], 1)


def _bits(w):
    return ((np.asarray(w)[:, None] >> np.arange(4)[None, :]) & 1) == 1


def _sum4(x):
    """[N, 4, 3] -> [N, 3] as (x_0 + x_1) + (x_2 + x_3)"""
    return (x[:, 0] + x[:, 1]) + (x[:, 2] + x[:, 3])


def estimate(P, dt_ctl, flat, q, v, contact, mask, normals, height, base, anchor, odo):
    """The law.  normals [N, 12] and height [N, 4], or both None.  -> dict(base [N, 6], anchor [N, 12], odo [N] int32, q_est, v_est; S, A, new: bool
    [N, 4] -- trusted, trusted with an anchor, anchored this tick; had: the in-bits)"""
    assert (normals is None) == (height is None)
    dt = q.dtype.type
    v, base, anchor = np.asarray(v, q.dtype), np.asarray(base, q.dtype), np.asarray(anchor, q.dtype)
    n = q.shape[0]
    lever, u = leg_terms(flat, q, v)
    S = _bits(contact) & _bits(mask)
    A = S & _bits(odo)
    inv = np.array([0, 1, 2, 3, 4], q.dtype)
    inv[1:] = dt(1) / inv[1:]
    cnt, na = S.sum(1), A.sum(1)
    ph, vh = base[:, 0:3].copy(), base[:, 3:6].copy()
    vm = -_sum4(np.where(S[:, :, None], u, dt(0))) * inv[cnt][:, None]
    vh = np.where((cnt > 0)[:, None], vh + dt(P["a_v"]) * (vm - vh), vh)
    pp = ph + dt(dt_ctl) * vh
    x = np.where(A[:, :, None], anchor.reshape(n, 4, 3) - lever, dt(0))
    pm = _sum4(x) * inv[na][:, None]
    ph = np.where((na > 0)[:, None], pp + dt(P["a_p"]) * (pm - pp), pp)
    new = S & ~A
    xa = ph[:, None, :] + lever
    if normals is not None:
        nr = np.asarray(normals, q.dtype).reshape(n, 4, 3)
        xa = xa - nr * ((nr * xa).sum(2) - np.asarray(height, q.dtype))[:, :, None]
    out_anchor = np.where(new[:, :, None], xa, anchor.reshape(n, 4, 3)).reshape(n, 12)
    w = (1 << np.arange(4))[None, :]
    out_odo = ((S * w).sum(1) | ((new * w).sum(1) << 4)).astype(np.int32)
    q_est, v_est = np.array(q), np.array(v)
    q_est[:, 0:3], v_est[:, 0:3] = ph, vh
    return dict(base=np.concatenate([ph, vh], 1), anchor=out_anchor, odo=out_odo, q_est=q_est, v_est=v_est, S=S, A=A, new=new, had=_bits(odo))


def estimate_loop(P, dt_ctl, flat, q, v, contact, mask, normals, height, base, anchor, odo):
    """estimate(), state by state and foot by foot in scalars of q's dtype: the statement of include/wbc_hip.h read line by line"""
    dt = q.dtype.type
    n = q.shape[0]
    lever, u = leg_terms(flat, q, v)
    base, anchor = np.array(base, q.dtype), np.array(anchor, q.dtype)
    out_odo = np.zeros(n, np.int32)
    q_est, v_est = np.array(q), np.array(v, q.dtype)
    for i in range(n):
        S = [bool((int(contact[i]) >> k) & (int(mask[i]) >> k) & 1) for k in range(4)]
        A = [S[k] and bool((int(odo[i]) >> k) & 1) for k in range(4)]
        cnt, na = sum(S), sum(A)
        for c in range(3):
            if cnt > 0:
                t = [u[i, k, c] if S[k] else dt(0) for k in range(4)]
                vm = -((t[0] + t[1]) + (t[2] + t[3])) * (dt(1) / dt(cnt))
                base[i, 3 + c] = base[i, 3 + c] + dt(P["a_v"]) * (vm - base[i, 3 + c])
            pp = base[i, c] + dt(dt_ctl) * base[i, 3 + c]
            if na > 0:
                t = [anchor[i, 3 * k + c] - lever[i, k, c] if A[k] else dt(0) for k in range(4)]
                pm = ((t[0] + t[1]) + (t[2] + t[3])) * (dt(1) / dt(na))
                pp = pp + dt(P["a_p"]) * (pm - pp)
            base[i, c] = pp
        word = 0
        for k in range(4):
            if not S[k]:
                continue
            word |= 1 << k
            if A[k]:
                continue
            x = base[i, 0:3] + lever[i, k]
            if normals is not None:
                nk = np.asarray(normals[i, 3 * k:3 * k + 3], q.dtype)
                x = x - nk * ((nk * x).sum() - dt(height[i, k]))
            anchor[i, 3 * k:3 * k + 3] = x
            word |= 16 << k
        out_odo[i] = word
        q_est[i, 0:3], v_est[i, 0:3] = base[i, 0:3], base[i, 3:6]
    return dict(base=base, anchor=anchor, odo=out_odo, q_est=q_est, v_est=v_est)


# ---- inputs that take every branch.  Per foot: (trusted, has an anchor) in all four combinations; per state: cnt = 0 .. 4, |A| = 0 with S != {}.
# State i takes S = i % 16 (every trust word) and the anchor word IN_OF[i % 16]; a foot outside S is untrusted for one of three reasons in turn
# (no contact, not in the mask, neither).  tests/test_odom_oracle.py asserts that every branch is taken.
IN_OF = tuple(7 if s == 7 else ((s << 1) | (s >> 3)) & 15 for s in range(16))     # S rotated by one foot; S = 7 keeps its own three
JUNK_BITS = 0x50        # bits outside 0-3 of contact, mask and odo: not read
BRANCH_DT = 2.0 ** -10


def branch_case(flat, total_mass, n, rank=0, planes=True, stand=True, states=None):
    """dict(q, v, contact, mask, normals, height (None without planes), base, anchor, odo, dt).  NaN in rows 0-2 of q and v and in the anchors of
    feet without an anchor bit; the anchors of the other feet lie within 2 cm of where the foot is.  stand: the synthetic model's standing posture
    (joints in leg-major order); False leaves synth.make_batch's joints, for other models.
    states: dict(q, v, normals (unit)) taken as it is instead of the drawn batch (tests/walk_edges.py): p_true is then the states' own base
    position, and every plane passes within 2 cm of its foot (height from the foot's own position: a plane through the origin would put a base
    50 m out 50 m from its ground)."""
    B = synth.make_batch(4, n, total_mass, rank=170 + rank) if states is None else states
    rng = np.random.default_rng(synth.SEED + 1700 + rank)
    q, v = B["q"].copy(), B["v"].copy()
    assert q.shape[0] == n
    if stand and states is None:
        q[:, 7:] += SR.loop_ref_params()["q_nom"] - np.tile(np.array(synth.NOMINAL_LEG), 4)
    i = np.arange(n)
    S = (i % 16).astype(np.int32)
    odo = np.array(IN_OF, np.int32)[i % 16]
    why = (i // 16 + i) % 3                     # of the feet outside S: 0 no contact, 1 not in the mask, 2 neither
    free = ~S & 15
    contact = S | np.where(why == 1, free, 0)
    mask = S | np.where(why == 0, free, 0)
    p_true = np.stack([rng.uniform(-1.0, 1.0, n), rng.uniform(-1.0, 1.0, n), rng.uniform(0.35, 0.45, n)], 1)
    if states is not None:
        p_true = q[:, 0:3].copy()
    lever, _ = leg_terms(flat, q, v)
    anchor = (p_true[:, None, :] + lever + rng.uniform(-0.02, 0.02, (n, 4, 3)))
    anchor[~_bits(odo)] = np.nan
    base = np.concatenate([p_true + rng.uniform(-0.01, 0.01, (n, 3)), rng.uniform(-0.3, 0.3, (n, 3))], 1)
    q[:, 0:3] = np.nan
    v[:, 0:3] = np.nan
    normals = B["normals"].copy() if planes else None
    height = rng.uniform(-0.02, 0.02, (n, 4)) if planes else None
    if planes and states is not None:
        height = height + (normals.reshape(n, 4, 3) * (p_true[:, None, :] + lever)).sum(2)
    return dict(q=q, v=v, contact=(contact | JUNK_BITS).astype(np.int32), mask=(mask | JUNK_BITS).astype(np.int32), normals=normals, height=height,
                base=base, anchor=anchor.reshape(n, 12), odo=(odo | JUNK_BITS).astype(np.int32), dt=BRANCH_DT)


def run(P, flat, c, fn=estimate, dtype=np.float64):
    """fn on a branch_case in dtype"""
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype)
    return fn(P, c["dt"], flat, f(c["q"]), f(c["v"]), c["contact"], c["mask"], f(c["normals"]), f(c["height"]), f(c["base"]), f(c["anchor"]), c["odo"])


def branches_taken(e):
    """set of (foot, 2 trusted + has an anchor on entry) over the states, plus ("cnt", c), ("na", c) and "fresh" (S != {} and A == {})"""
    seen = set()
    for k in range(4):
        seen |= {(k, int(b)) for b in np.unique(2 * e["S"][:, k] + e["had"][:, k])}
    seen |= {("cnt", int(c)) for c in np.unique(e["S"].sum(1))} | {("na", int(c)) for c in np.unique(e["A"].sum(1))}
    if np.any((e["S"].sum(1) > 0) & (e["A"].sum(1) == 0)):
        seen.add("fresh")
    return seen


ALL_BRANCHES = {(k, b) for k in range(4) for b in range(4)} | {("cnt", c) for c in range(5)} | {("na", c) for c in range(5)} | {"fresh"}


def written(e):
    """bool [N, 12]: the anchor words the call wrote"""
    return np.repeat(e["new"], 3, axis=1)


# estimate() in float32 against float64 on branch_case(n, rank=n) of PARITY_SIZES with and without planes (synthetic model, default parameters): the
# largest error relative to the largest entry of the array, rounded up to two digits -- what single precision costs.  tests/test_odom_oracle.py
# checks the numbers, tests/test_gpu_odom.py gates the device's fp32 results at F32_MARGIN x them (the margin of the gait tests).
F32_ERR = dict(p=8.0e-8, v=9.5e-8, anchor=1.1e-7)
F32_MARGIN = 8.0


def f32_errors(flat, total_mass):
    """the measurement behind F32_ERR; asserts on the way that float32 forms the same integer words and leaves the same words untouched"""
    P = params()
    worst = dict(p=0.0, v=0.0, anchor=0.0)
    for n in PARITY_SIZES:
        for planes in (True, False):
            c = branch_case(flat, total_mass, n, rank=n, planes=planes)
            e64, e32 = run(P, flat, c), run(P, flat, c, dtype=np.float32)
            assert np.array_equal(e32["odo"], e64["odo"])
            w = written(e64)
            assert np.array_equal(e32["anchor"][~w], c["anchor"].astype(np.float32)[~w], equal_nan=True)
            rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max()) if b.size else 0.0
            worst["p"] = max(worst["p"], rel(e32["base"][:, 0:3], e64["base"][:, 0:3]))
            worst["v"] = max(worst["v"], rel(e32["base"][:, 3:6], e64["base"][:, 3:6]))
            worst["anchor"] = max(worst["anchor"], rel(e32["anchor"][w], e64["anchor"][w]))
    return worst


# ---- the walking loop on the estimated base state
WALK_N = 4
NAN3 = np.full(3, np.nan)


def walk_case(flat, oracle, n=WALK_N):
    return stick_ref.walk_case(flat, oracle, n)


def closed_loop(flat, oracle, case, sensed="estimate", planes=True, P=None, ticks=GND.WALK_TICKS, k_t=stick_ref.DEFAULT_KT, q0=None, estimated=True):
    """walk_ref.closed_loop's links in its order, on the stiction plant with the observer on, with the base estimate in front:
        estimate(contact, mask as the last tick left them) -> gait -> oracle.reference -> swing_reference -> oracle.step -> contact_ref.estimate -> plant
    The controller links (the first six) get q_est, v_est and the dynamics at them; the plant integrates the TRUE state with the M, h, Jc the step
    formed, as the device tick does.  The law's q and v carry NaN in rows 0-2.
    sensed     "estimate": the gait rule gets the word formed after the last step and the law the word before that one (the word gait_estimated_odom
               loads); "plant": both get the plant's word of the last tick
    planes     the law gets the tick's normals and height, or neither
    estimated  False: the controller links get the true q, v (the law still runs beside them: its errors are those of an estimator nobody listens to)
    Returns dict(q, v at the end; q0; status_ok; perr, verr [ticks, N, 3]: estimate - truth at the state every tick started from; base, anchor, odo at
    the end; masks, events, odos [ticks, N]; contacts: the estimated words)"""
    assert sensed in ("estimate", "plant")
    P = P or params()
    CP, GP = contact_ref.params(), GR.walk_params(flat)
    prm, G = synth.default_params(observer_order=1), SR.loop_ref_params()
    prm["dt"] = GR.DYADIC_DT
    legs = limit_ref.leg_joints(flat)
    plant = walk_ref.ground_plant(flat, case, GND.params(), k_t)
    q, v = (case["q"] if q0 is None else q0).copy(), case["v"].copy()
    start = q.copy()
    n = q.shape[0]
    phase, mask, swing = case["phase"].copy(), case["mask"].copy(), case["swing"].copy()
    contact, est, est_prev = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    integ, r = np.ascontiguousarray(oracle.dynamics(q, v)["p"]), np.zeros((n, 18))
    tau_prev, f_prev = np.zeros((n, 12)), np.zeros((n, 12))
    base, anchor, odo = np.concatenate([q[:, 0:3], v[:, 0:3]], 1), np.zeros((n, 12)), np.zeros(n, np.int32)
    rec = dict(perr=[], verr=[], masks=[], events=[], odos=[], contacts=[])
    ok = True
    for k in range(ticks):
        height = case["height0"] if k < GND.BUMP_TICK else case["height1"]
        qs, vs = q.copy(), v.copy()
        qs[:, 0:3], vs[:, 0:3] = NAN3, NAN3
        o = estimate(P, prm["dt"], flat, qs, vs, est_prev if sensed == "estimate" else contact, mask, case["normals"] if planes else None,
                     height if planes else None, base, anchor, odo)
        base, anchor, odo = o["base"], o["anchor"], o["odo"]
        rec["perr"].append(base[:, 0:3] - q[:, 0:3]); rec["verr"].append(base[:, 3:6] - v[:, 0:3]); rec["odos"].append(odo.copy())
        qe, ve = (o["q_est"], o["v_est"]) if estimated else (q, v)
        phase, mask, swing, ev = GR.gait_tick(flat, GP, prm["dt"], qe, ve, case["cmd"], est if sensed == "estimate" else contact, phase, mask, swing)
        rec["masks"].append(mask.copy()); rec["events"].append(ev.copy())
        ref = oracle.reference(G, qe, ve, case["plan"], k * prm["dt"])
        vd, _ = SR.swing_reference(flat, qe, ve, mask, swing, 0.0, ref["vdot_des"], GR.WALK_SWING_PARAMS)
        tick = oracle.step(prm, qe, ve, ref["w_des"], vd, case["normals"], case["mu"], mask, tau_prev, f_prev, integ, r)
        ok = ok and bool(np.all(tick["status"] == 0))
        dyn = oracle.dynamics(qe, ve)
        e = contact_ref.estimate(CP, dyn["Jc"], r, f_prev, case["normals"], est, legs)
        est_prev, est = est, e["contact"]
        rec["contacts"].append(est.copy())
        tau_prev, f_prev = tick["tau"], tick["f"]
        q, v, g = plant(k, prm, dyn, tick, q, v)
        contact = g["contact"]
    out = dict(q=q, v=v, q0=start, status_ok=ok, base=base, anchor=anchor, odo=odo, mask=mask, swing=swing, phase=phase)
    out.update({key: np.array(val) for key, val in rec.items()})
    return out


def figures(w):
    """dict(travel [N] (m, forward), base_z [N] at the end, perr [3]: the worst |p^ - p| per axis, vrms [3]: the rms velocity error per axis)"""
    return dict(travel=w["q"][:, 0] - w["q0"][:, 0], base_z=w["q"][:, 2].copy(), perr=np.abs(w["perr"]).max((0, 1)),
                vrms=np.sqrt((w["verr"] ** 2).mean((0, 1))))


def cpu_walk(flat, oracle, sensed="estimate", planes=True, estimated=True, n=WALK_N):
    """(case, closed_loop(case, ...)) of n robots, computed once per process and shared by the tests that need it: read only"""
    return walk_ref.cached(("odom", id(flat), n, sensed, planes, estimated), lambda: walk_case(flat, oracle, n),
                           lambda case: closed_loop(flat, oracle, case, sensed, planes, estimated=estimated))


# Measured with closed_loop (n = 4, default parameters, planes given; tests/test_odom_oracle.py asserts them) against the same loop with the controller
# links on the true state (estimated = False), per contact word.  Every band is a factor 2 around the measurement, as contact_ref.BASE_Z_BAND is.
#   the true-state loops    travel 4.95 .. 5.12 cm, base z at the end 0.4024 .. 0.4033 m (both words)
#   "estimate"              travel 3.47 .. 5.41 cm, base z 0.3937 .. 0.4103 m;  worst |p^ - p| 31.3 / 5.7 / 8.9 mm;  rms v error 0.063 / 0.033 / 0.063 m/s
#   "plant"                 travel 3.02 .. 5.57 cm, base z 0.3969 .. 0.4181 m;  worst |p^ - p| 38.0 / 5.7 / 7.7 mm;  rms v error 0.072 / 0.034 / 0.043 m/s
# Where the x error comes from (robot 0, whose foot 1 meets the 15 mm bump): that foot lands early, is loaded with 40 N and SLIDES at 0.5 .. 0.2 m/s for
# thirty ticks while the law trusts it; and the estimated word of a foot the schedule has just put down carries the planned force, so its bit is set one
# or two ticks before the foot is down.  Each anchor taken from a moving foot keeps its error.  y and z stay within one penetration depth.
# Without planes the new anchors keep the foot's penetration: z reads 15 .. 19 mm high at the end (5 mm with planes) and the worst z error is 20.5 mm.
TRAVEL_BAND = dict(estimate=2 * 1.52e-2, plant=2 * 1.96e-2)       # m; |forward travel, estimated loop - true-state loop|, per robot
BASE_Z_BAND = dict(estimate=2 * 8.7e-3, plant=2 * 1.5e-2)         # m; |base z at the end, estimated loop - true-state loop|
PERR_BAND = dict(estimate=(2 * 3.14e-2, 2 * 5.7e-3, 2 * 9.0e-3), plant=(2 * 3.81e-2, 2 * 5.7e-3, 2 * 7.8e-3))      # m; worst |p^ - p| per axis
NO_PLANES_Z = 2.0            # the worst z error without planes is more than this many times the one with planes (measured 2.3 / 2.7)
# amplification of a 1e-12 relative perturbation of q0 over the estimated loop ("estimate", planes): measured 17.7 (q) and 1404 (v: the estimated
# velocity is rough and the swing gains are stiff), rounded up by the factor 2 of the contact loop's.  The device loop's gate in
# tests/test_gpu_odom.py is max(1e-6, 10 A 1e-9), the rule of tests/test_gpu_ground.py.
WALK_AMPLIFICATION = dict(q=36.0, v=2800.0)
