"""Gait scheduler (wbc_gait_batch, include/wbc_hip.h "Gait scheduler") restated in numpy, for the tests (test infrastructure).

Works on the flat model of oracle/urdf_model.py in the dtype of q, like tests/swing_ref.py, so that the same code evaluated in float32 measures what
single precision costs (tests/test_gpu_gait.py, F32_GATE).  Row-per-state arrays: q [N, 19], v [N, 18], cmd [N, 4], phase [N], mask [N], swing [N, 36].
  host_consts   dphi, inv_sw, T_sw as the host forms them: in double, rounded to the scalar type
  gait_tick     the call itself: (phase, mask, swing, events) of the next tick; the arguments are not modified
  base_xy       the default nominal footholds (hip origins) of a flat model
  branch_case   a batch that takes every branch of the mask rule for every foot, with every phase away from the switching points
  walk_case / closed_loop   the CPU loop gait -> oracle.reference -> swing_reference -> oracle.step -> limit_ref.integrate
"""
import numpy as np

from tests import swing_ref as SR, walk_ref
from wbc_quadruped_dob_amd import synth

DEFAULT_PARAMS = dict(period=0.4, duty=(0.6,) * 4, offset=(0.0, 0.5, 0.5, 0.0), clearance=0.05, k_v=0.03, late=0.5, retarget=1)
DYADIC = dict(period=2.0 ** -2, duty=(0.5,) * 4, offset=(0.0, 0.5, 0.5, 0.0))   # with dt = 2^-10: dphi = 2^-8, every phase a dyadic number
DYADIC_DT = 2.0 ** -10


def base_xy(flat):
    """[4, 2]: x, y of the origin of the first joint of every foot's leg in the base frame (wbc_gait_params_default)"""
    return np.array([np.asarray(flat["rt"], np.float64).reshape(-1, 3)[SR._chain(flat, k)[0]][:2] for k in range(len(flat["foot_body"]))])


def params(flat, **kw):
    P = dict(DEFAULT_PARAMS, base_xy=base_xy(flat))
    for k, val in kw.items():
        assert k in P, k
        P[k] = val
    P["duty"] = tuple(np.broadcast_to(np.asarray(P["duty"], np.float64), (4,)))
    P["offset"] = tuple(np.broadcast_to(np.asarray(P["offset"], np.float64), (4,)))
    return P


def host_consts(P, dt_ctl, dtype):
    """dphi, inv_sw [4], T_sw [4]: formed in double, rounded to dtype"""
    t = np.dtype(dtype).type
    duty = np.asarray(P["duty"], np.float64)
    inv = np.array([0.0 if d == 1.0 else 1.0 / (1.0 - d) for d in duty])
    return t(dt_ctl / P["period"]), inv.astype(dtype), ((1.0 - duty) * P["period"]).astype(dtype)


def gait_tick(flat, P, dt_ctl, q, v, cmd, contact, phase, mask, swing):
    """-> (phase', mask', swing', events); arithmetic in q's dtype, the operation order of the header's steps 1 .. 5"""
    dt = q.dtype
    t = dt.type
    v, cmd, phase, swing = np.asarray(v, dt), np.asarray(cmd, dt), np.asarray(phase, dt), np.array(swing, dt)
    mask = np.asarray(mask)
    contact = np.zeros_like(mask) if contact is None else np.asarray(contact)
    dphi, inv_sw, T_sw = host_consts(P, dt_ctl, dt)
    one = t(1)
    ph = phase + dphi
    ph = np.where(ph >= one, ph - one, ph).astype(dt)
    R = SR._quat_R(q[:, 3:7])
    hn = one / np.sqrt(R[:, 0, 0] * R[:, 0, 0] + R[:, 1, 0] * R[:, 1, 0])
    hx, hy = R[:, 0, 0] * hn, R[:, 1, 0] * hn
    cx, cy = hx * cmd[:, 0] - hy * cmd[:, 1], hy * cmd[:, 0] + hx * cmd[:, 1]
    new_mask = np.zeros_like(mask)
    events = np.zeros_like(mask)
    for k in range(4):
        duty, off = t(P["duty"][k]), t(P["offset"][k])
        pk = ph + off
        pk = np.where(pk >= one, pk - one, pk).astype(dt)
        sched = pk < duty
        u = ((pk - duty) * inv_sw[k]).astype(dt)
        was = ((mask >> k) & 1) == 1
        sensed = ((contact >> k) & 1) == 1
        late = u >= t(P["late"])
        bit = sched | (late & (was | sensed))
        lift, touch = was & ~bit, ~was & bit
        new_mask |= bit.astype(mask.dtype) << k
        events |= (lift.astype(mask.dtype) << k) | (touch.astype(mask.dtype) << (4 + k))
        nx, ny = t(P["base_xy"][k][0]), t(P["base_xy"][k][1])
        bx, by = hx * nx - hy * ny, hy * nx + hx * ny
        Trem = (one - u) * T_sw[k]
        hst = t(0.5) * (duty * t(P["period"]))
        kv = t(P["k_v"])
        p1 = np.stack([q[:, 0] + bx + v[:, 0] * Trem + hst * cx + kv * (v[:, 0] - cx) + hst * cmd[:, 2] * (-by),
                       q[:, 1] + by + v[:, 1] * Trem + hst * cy + kv * (v[:, 1] - cy) + hst * cmd[:, 2] * bx,
                       cmd[:, 3]], 1).astype(dt)
        sw = swing[:, 9 * k:9 * k + 9]      # a view: writes land in `swing`
        if lift.any():
            sw[lift, 0:3] = SR.foot_kin(flat, k, q[lift], v[lift])["pf"]
        sw[lift, 6], sw[lift, 7] = t(P["clearance"]), T_sw[k]
        air = ~bit
        sw[air, 8] = (u * T_sw[k])[air]
        new_p1 = air if P["retarget"] else lift
        sw[new_p1, 3:6] = p1[new_p1]
    return ph, new_mask, swing, events


def switching_distance(P, dt_ctl, phase):
    """[N]: the smallest distance of any foot's NEXT phase phi_k from a switching point (0, duty, duty + late (1 - duty), 1), in float64"""
    ph = (np.asarray(phase, np.float64) + dt_ctl / P["period"]) % 1.0
    out = np.full(ph.shape, np.inf)
    for k in range(4):
        pk = (ph + P["offset"][k]) % 1.0
        d = P["duty"][k]
        for x in (0.0, d, d + P["late"] * (1.0 - d), 1.0):
            out = np.minimum(out, np.abs(pk - x))
    return out


def branch_case(flat, total_mass, n, rank=0, P=None, dt_ctl=1e-3):
    """synth.make_batch states (generic attitudes), commands with all four rows non-zero, swing words filled with recognisable junk, and per state a
    (phase, previous mask, contact) triple out of a table that -- for EVERY foot -- takes every branch of the mask rule: scheduled stance from stance
    and from swing; lift-off; a stance foot late in its window staying down; a continuing swing with and without contact before and after `late`
    (early touchdown).  Every state's phases keep 1e-3 clear of the switching points (asserted).  dict(q, v, cmd, contact, phase, mask, swing)"""
    P = P or params(flat)
    B = synth.make_batch(3, n, total_mass, rank=90 + rank)
    rng = np.random.default_rng(synth.SEED + 1100 + rank)
    # phases (before the tick) that put each foot early and late in its swing window and early and late in stance, for both offset groups
    phases = (0.05, 0.17, 0.33, 0.45, 0.55, 0.67, 0.83, 0.95, 0.62, 0.78, 0.12, 0.28)
    table = [dict(phase=np.array([p]), mask=np.array([m], np.int32), contact=np.array([c], np.int32))
             for p in phases for m in (0b1111, 0b0000, 0b1001, 0b0110, 0b0101) for c in (0b0000, 0b1111, 0b0101, 0b1010)]
    # greedy cover: the rows that add the most (foot, branch) pairs not seen yet come first, the rest of the batch cycles through the table
    rows, seen = [], set()
    while len(seen) < len(ALL_BRANCHES):
        best = max(table, key=lambda r: len(branches_taken(P, dt_ctl, [r]) - seen))
        assert branches_taken(P, dt_ctl, [best]) - seen
        rows.append(best); seen |= branches_taken(P, dt_ctl, [best])
    rows = (rows + [table[(i * 37 + rank * 11) % len(table)] for i in range(n)])[:n]
    phase, mask, contact = (np.concatenate([r[k] for r in rows]) for k in ("phase", "mask", "contact"))
    assert np.all(switching_distance(P, dt_ctl, phase) > 1e-3)
    cmd = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-1.0, 1.0, (n, 1)), rng.uniform(-0.05, 0.05, (n, 1))], 1)
    swing = rng.uniform(-1.0, 1.0, (n, SR.SWING_WORDS))
    return dict(q=B["q"], v=B["v"], cmd=cmd, contact=contact, phase=phase, mask=mask, swing=swing)


def branches_taken(P, dt_ctl, cases):
    """set of (foot, branch) over a list of cases, evaluated in float64; the branches of the mask rule are
    0 scheduled from stance, 1 scheduled from swing (touchdown), 2 lift-off, 3 stance foot late in its window stays down,
    4 early touchdown, 5 contact before `late` ignored, 6 swing continues without contact after `late`, 7 ... before `late`"""
    seen = set()
    for c in cases:
        ph = (c["phase"] + dt_ctl / P["period"]) % 1.0
        for k in range(4):
            pk = (ph + P["offset"][k]) % 1.0
            sched = pk < P["duty"][k]
            late = (pk - P["duty"][k]) / max(1.0 - P["duty"][k], 1e-300) >= P["late"]
            was, sensed = ((c["mask"] >> k) & 1) == 1, ((c["contact"] >> k) & 1) == 1
            br = np.where(sched, np.where(was, 0, 1), np.where(was, np.where(late, 3, 2), np.where(sensed, np.where(late, 4, 5), np.where(late, 6, 7))))
            seen |= {(k, int(x)) for x in br}
    return seen


ALL_BRANCHES = {(k, b) for k in range(4) for b in range(8)}


PARITY_SIZES = (1, 15, 16, 17, 33)
# gait_tick in float32 against float64 on branch_case(n, rank=n) of PARITY_SIZES (synthetic model, default parameters), largest error relative to the
# largest entry of the array, rounded up to two digits: what single precision costs.  tests/test_gait_oracle.py checks the numbers, tests/test_gpu_gait.py
# gates the device's fp32 results at 8 x them.
F32_ERR = dict(phase=4.0e-8, p0=1.5e-7, p1=1.7e-7, t0=2.6e-7)


def written_words(mask, events, retarget=1):
    """bool [N, 36] x 4: the words of p0 / p1 / t0 / (hgt, T) a call with these results wrote"""
    n = len(mask)
    p0, p1, t0, ht = (np.zeros((n, SR.SWING_WORDS), bool) for _ in range(4))
    for k in range(4):
        air = ((mask >> k) & 1) == 0
        lift = ((events >> k) & 1) == 1
        p0[lift, 9 * k:9 * k + 3] = True
        ht[lift, 9 * k + 6:9 * k + 8] = True
        p1[air if retarget else lift, 9 * k + 3:9 * k + 6] = True
        t0[air, 9 * k + 8] = True
    return p0, p1, t0, ht


def f32_errors(flat, total_mass, dt_ctl=1e-3):
    """the measurement behind F32_ERR; asserts on the way that float32 takes the same branches as float64 on every state of the cases"""
    P = params(flat)
    worst = dict(phase=0.0, p0=0.0, p1=0.0, t0=0.0)
    f = lambda a: a.astype(np.float32)
    for n in PARITY_SIZES:
        c = branch_case(flat, total_mass, n, rank=n, P=P, dt_ctl=dt_ctl)
        r64 = gait_tick(flat, P, dt_ctl, c["q"], c["v"], c["cmd"], c["contact"], c["phase"], c["mask"], c["swing"])
        r32 = gait_tick(flat, P, dt_ctl, f(c["q"]), f(c["v"]), f(c["cmd"]), c["contact"], f(c["phase"]), c["mask"], f(c["swing"]))
        assert np.array_equal(r32[1], r64[1]) and np.array_equal(r32[3], r64[3])
        p0, p1, t0, _ = written_words(r64[1], r64[3])
        worst["phase"] = max(worst["phase"], float(np.abs(r32[0] - r64[0]).max() / np.abs(r64[0]).max()))
        for what, w in (("p0", p0), ("p1", p1), ("t0", t0)):
            if w.any():
                worst[what] = max(worst[what], float(np.abs(r32[2][w] - r64[2][w]).max() / np.abs(r64[2][w]).max()))
    return worst


def exact_schedule(flat, dtype, n, ticks=512, phase0=None):
    """The dyadic trot (DYADIC, dt = 2^-10) on n standing robots for `ticks` ticks in `dtype`: every number the mask depends on is a dyadic rational, so
    float32 and float64 give the same masks.  dict(q, v, cmd: the inputs (float64); phase0, phase; masks, events [ticks, n]; swing at the end)"""
    G = SR.loop_ref_params()
    rng = np.random.default_rng(synth.SEED + 1200)
    q = np.zeros((n, 19)); q[:, 2] = 0.40; q[:, 6] = 1.0
    q[:, 7:] = G["q_nom"] + rng.uniform(-0.03, 0.03, (n, 12))
    v = np.zeros((n, 18))
    cmd = np.tile([0.25, 0.0, 0.0, -0.0625], (n, 1))
    P = params(flat, **DYADIC)
    phase0 = np.zeros(n, dtype) if phase0 is None else np.asarray(phase0, dtype)
    phase, mask, swing = phase0.copy(), np.full(n, 0b1111, np.int32), np.zeros((n, SR.SWING_WORDS), dtype)
    qd, vd, cd = q.astype(dtype), v.astype(dtype), cmd.astype(dtype)
    masks, events = [], []
    for _ in range(ticks):
        phase, mask, swing, ev = gait_tick(flat, P, DYADIC_DT, qd, vd, cd, None, phase, mask, swing)
        masks.append(mask.copy()); events.append(ev.copy())
    return dict(q=q, v=v, cmd=cmd, phase0=phase0, phase=phase, masks=np.array(masks), events=np.array(events), swing=swing)


# ---- the closed loop: gait -> reference -> swing reference -> tick -> plant, per tick
WALK_SPEED, WALK_TICKS = 0.1, 512     # commanded forward speed (m/s); two periods of the dyadic trot at dt = 2^-10
# The swing gains of the walking loop.  A swing of this trot lasts 0.125 s; with the default gains (kp 400: a closed-loop time constant of 50 ms) and
# the commanded 0.2 m/s the feet land 0.04 .. 0.47 of their step away from p1 (16 robots, CPU loop).  Stiffer, still critically damped gains and half
# the speed bring the worst landing to 0.070 of its step (0.2 m/s with these gains: 0.115; 0.1 m/s with kp 2500, kd 100: 0.088).
WALK_SWING_PARAMS = dict(kp=(4900.0,) * 3, kd=(140.0,) * 3)


def walk_params(flat):
    return params(flat, **DYADIC)


def walk_case(flat, oracle, n):
    """n robots standing in swing_ref.loop_ref_params' posture (small per-robot differences), all feet down, phase 0; the command is WALK_SPEED forward
    on the ground the feet stand on, and the CoM plan moves the CoM forward at that speed: WALK_SPEED * duration over the loop's duration.
    dict(q, v, cmd, phase, mask, swing, plan, normals, mu)"""
    c = SR.loop_case(flat, oracle, n)
    dur = WALK_TICKS * DYADIC_DT
    c["plan"][:, 3] += WALK_SPEED * dur
    c["plan"][:, 6] = dur
    zg = np.mean([SR.foot_kin(flat, k, c["q"], c["v"])["pf"][:, 2] for k in range(4)], 0)
    c["cmd"] = np.stack([np.full(n, WALK_SPEED), np.zeros(n), np.zeros(n), zg], 1)
    c["phase"] = np.zeros(n)
    c["mask"] = np.full(n, 0b1111, np.int32)
    c["swing"] = np.zeros((n, SR.SWING_WORDS))
    return c


def closed_loop(flat, oracle, case, ticks=WALK_TICKS, P=None, swing_params=None):
    """CPU loop.  Returns dict(q, v, foot at the end; masks, events [ticks, N]; status_ok; landings: list of (tick, state, foot, |p1 - p0|, |p_f - p1|) at
    every touchdown, p_f the foot position the gait call of that tick saw)."""
    P = P or walk_params(flat)
    swing_params = WALK_SWING_PARAMS if swing_params is None else swing_params
    landings = []
    extras = lambda now: landings.extend(landings_of(flat, now["k"], now["q"], now["v"], now["swing"], now["events"]))
    w = walk_ref.closed_loop(flat, oracle, case, ticks, walk_ref.rigid_plant(), swing_params, gait=P, extras=extras)
    return dict(q=w["q"], v=w["v"], foot=SR.foot_words(flat, w["q"], w["v"]), masks=w["masks"], events=w["events"], status_ok=w["status_ok"],
                landings=landings, phase=w["phase"], swing=w["swing"])


def cpu_walk(flat, oracle, n):
    """(case, closed_loop(case)) of n robots, computed once per process and shared by the tests that need it: read only"""
    return walk_ref.cached(("gait", id(flat), n), lambda: walk_case(flat, oracle, n), lambda case: closed_loop(flat, oracle, case))


def landing_ratios(landings, min_step=0.02):
    """|p_f - p1| / |p1 - p0| of every touchdown whose step is at least min_step"""
    return np.array([L[4] / L[3] for L in landings if L[3] >= min_step])


def landings_of(flat, tick, q, v, swing, ev):
    """touchdowns of this tick: (tick, state, foot, |p1 - p0|, |p_f - p1|) with the plan words as they stand (a landed foot's are no longer written)"""
    out = []
    for f in range(4):
        for s in np.nonzero((ev >> (4 + f)) & 1)[0]:
            pf = SR.foot_kin(flat, f, q[s:s + 1], v[s:s + 1])["pf"][0]
            p0, p1 = swing[s, 9 * f:9 * f + 3], swing[s, 9 * f + 3:9 * f + 6]
            out.append((tick, int(s), f, float(np.linalg.norm(p1 - p0)), float(np.linalg.norm(pf - p1))))
    return out
