"""Robot states OUTSIDE the narrow kinematic box of synth.make_batch, for tests/test_envelope_oracle.py (CPU) and tests/test_gpu_envelope.py (GPU).
Test infrastructure.

synth.make_batch draws joints within 0.3 rad of the nominal stance, attitudes within 0.3 rad of upright (quaternion w > 0), base x = y = 0 and base
angular velocities of 0.5 rad/s at dt = 1e-3.  The builders here start from such a batch and overwrite ONLY the kinematic words:
  wide_batch    joints over +- 7 pi with exact multiples of pi/4 (every quadrant of the device's sincos, both signs, the ties of rint), attitudes
                uniform on the sphere with exact half turns (w = 0) and yaw +- pi/2 in the first rows, base x, y over +- 50 m
  far_joints    joint angles over the documented range of the device's sincos (+- 1e5 rad in fp64, +- 1e4 rad in fp32), rounded to the scalar type
  spin_batch    base angular velocities whose step angle theta = |omega| dt spans 0 ... 1.5 rad in every group of 16 states (the fp32 quaternion step
                switches from its power series to the closed form at theta = 0.5), with omega = 0 and theta = 0.5 -+ 5e-4 among them
  wide_swing_case / wide_branch_case   swing_ref.swing_case / gait_ref.branch_case on wide states
  integrate_ref the plant step restated with numpy's LU and crosscheck_np.integrate_q, float64
The F32_* constants are what float32 costs on these inputs, measured on the CPU by tests/test_envelope_oracle.py (which also checks them); the GPU file
gates the device's fp32 swing and gait results at 8 x them, the convention of gait_ref.F32_ERR.
"""
import numpy as np

from oracle import crosscheck_np as X
from tests import gait_ref as GR, limit_ref, swing_ref as SR
from wbc_quadruped_dob_amd import synth

LAYERS = ("joints", "attitude", "position")
SIZES = (1, 17, 65, 130, 258)       # ragged against 16-, 32- and 64-state groups; the even ones serve the packed fp32 sweep
JOINT_SPAN = 7.0 * np.pi            # reduction counts n = rint(x 2 / pi) from -14 to 14: every residue mod 4, both signs, several turns
SNAP_SHARE = 0.15
BASE_SPAN = 50.0                    # m
FAR_SPAN = {np.float64: 1e5, np.float32: 1e4}     # the ranges the comments of csrc/dyn_sweep.hip.hpp state for sincos_t
HEADING_MIN = 0.01                  # gait cases skip states with R00^2 + R10^2 below this: the Raibert frame divides by its root
HEADING_SKIP_CAP = 0.02             # ... at most this share of a case
SPIN_DT, SPIN_THETA_MAX, SPIN_SWITCH = 0.02, 1.5, 0.5

# float32 against float64 of tests/swing_ref.py and tests/gait_ref.py on wide_swing_case(n, rank=n) / wide_branch_case(n, rank=n) of SIZES, largest
# error relative to the largest entry of the array, rounded up to two digits (tests/test_envelope_oracle.py prints and checks them)
F32_SWING = dict(vdot=1.9e-3, foot=1.6e-7)      # (vdot: the near-singular legs of random postures carry it; the narrow envelope has 7.4e-6)
F32_GAIT = dict(phase=4.0e-8, p0=1.3e-7, p1=1.7e-7, t0=2.6e-7)
# ... and of oracle.reference on reference_case(n) of REFERENCE_SIZES.  The narrow envelope's fp32 gate of tests/test_gpu_reference.py (2e-5) does not carry
# over: 50 m from the origin the PD terms kp (plan - c) cancel two numbers of magnitude 50, and the fp32 oracle itself is 3.5e-5 off the fp64 one in w_des
F32_REFERENCE = dict(w_des=3.5e-5, vdot_des=2.1e-7, com=1.8e-7)
REFERENCE_SIZES, REFERENCE_T = (17, 130), 0.017

# The tick cases of tests/test_gpu_envelope.py, one per kernel family the planner can return, forced at these sizes with the options the older GPU tests
# use: (id, dtype, observer order, config, n, options, want_mats, the fields of wbc_tick_plan the case must show).  All three layers, rank = n.
TICK_CASES = (
    ("fused-1", "f64", 0, 2, 1, {}, True, dict(fused=1)),
    ("fused", "f64", 1, 3, 65, {}, True, dict(fused=1)),
    ("fused-f32", "f32", 2, 4, 130, {}, True, dict(fused=1)),
    ("pair", "f64", 0, 2, 65, {"fused_pair": 1}, True, dict(fused=3)),
    ("pair-f32", "f32", 0, 3, 130, {"fused_pair": 1}, True, dict(fused=3)),
    ("tile-f64-obs0", "f64", 0, 2, 65, {"tile_tick": 1, "fused_max": 0}, True, dict(fused=2, front=0, qp_body=2)),
    ("tile-f64-obs1", "f64", 1, 4, 65, {"tile_tick": 1, "fused_max": 0}, True, dict(fused=2, front=4, qp_body=2)),
    ("tile-f32-obs0", "f32", 0, 3, 258, {"tile_tick": 1, "fused_max": 0}, True, dict(fused=2, front=0, sweep_pack2=1)),
    ("tile-f32-obs1", "f32", 1, 4, 130, {"tile_tick": 1, "fused_max": 0}, True, dict(fused=2, front=4, sweep_pack2=1)),
    ("two-onewave", "f64", 2, 4, 65, {"fused_max": 0, "qp_tile": -1}, True, dict(fused=0, front=0, qp=0)),
    ("two-qptile64", "f64", 0, 3, 130, {"fused_max": 0, "qp_tile": 64}, True, dict(fused=0, front=0, qp=1, qp_tile=64)),
    ("two-qptile64-f32", "f32", 1, 4, 130, {"fused_max": 0, "qp_tile": 64, "tile_tick": -1}, True, dict(fused=0, qp=1, qp_tile=64, qp_body=2)),
    ("two-lane", "f64", 1, 3, 258, {"fused_max": 0, "qp_lane": 1}, True, dict(fused=0, qp=2)),
    ("two-pack2-f32", "f32", 0, 2, 258, {"fused_max": 0, "f32_pack2": 1, "tile_tick": -1}, True, dict(fused=0, sweep_pack2=1)),
    ("two-unpacked-f32", "f32", 1, 3, 65, {"fused_max": 0}, True, dict(fused=0, sweep_pack2=0)),
    ("obs-split", "f64", 1, 4, 17, {"fused_max": 0, "obs_split_min": 1}, True, dict(fused=0, front=2)),
    ("obs-split-f32", "f32", 2, 4, 130, {"fused_max": 0, "obs_split_min": 1}, True, dict(fused=0, front=2)),
    ("rnea", "f64", 0, 3, 65, {"fused_max": 0}, False, dict(fused=0, front=1)),
    ("rnea-obs2", "f64", 2, 4, 1, {}, False, dict(fused=0, front=1)),
)

EDGE_QUATS = np.array([[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0],                  # half turns about x, y, z: w = 0
                       [0.0, 0.0, np.sqrt(0.5), np.sqrt(0.5)], [0.0, 0.0, -np.sqrt(0.5), np.sqrt(0.5)]])  # yaw + pi/2, - pi/2


def _rng(cfg, n, rank, salt):
    return np.random.default_rng(synth.SEED + 0xE7E + 7919 * salt + 1000 * cfg + 31 * rank + n)


def wide_joints(rng, n, nj=12):
    """[n, nj] uniform in +- 7 pi, about 15 % of the entries snapped to exact multiples k pi/4, k in -28 ... 28 (as exact as float64 has them)"""
    j = rng.uniform(-JOINT_SPAN, JOINT_SPAN, (n, nj))
    snap = rng.random((n, nj)) < SNAP_SHARE
    k = rng.integers(-28, 29, (n, nj))
    return np.where(snap, k * (np.pi / 4), j)


def wide_quats(rng, n):
    """[n, 4] unit quaternions (x, y, z, w) uniform on the sphere; the first rows, where present, are EDGE_QUATS"""
    qq = rng.normal(size=(n, 4))
    qq /= np.linalg.norm(qq, axis=1, keepdims=True)
    m = min(n, len(EDGE_QUATS))
    qq[:m] = EDGE_QUATS[:m]
    return qq


def wide_batch(cfg, n, total_mass, rank=0, layers=LAYERS):
    """synth.make_batch(cfg, n, total_mass, rank) with the kinematic words of the named layers overwritten; everything else as it was"""
    assert set(layers) <= set(LAYERS), layers
    B = synth.make_batch(cfg, n, total_mass, rank)
    q = B["q"]
    # (each layer from its own stream: a single-layer batch and the all-layer batch of the same arguments share that layer's numbers)
    if "joints" in layers:
        q[:, 7:] = wide_joints(_rng(cfg, n, rank, 1), n, q.shape[1] - 7)
    if "attitude" in layers:
        q[:, 3:7] = wide_quats(_rng(cfg, n, rank, 2), n)
    if "position" in layers:
        q[:, 0:2] = _rng(cfg, n, rank, 3).uniform(-BASE_SPAN, BASE_SPAN, (n, 2))
    return B


def far_joints(n, dtype, rank=0, nj=12):
    """[n, nj] joint angles uniform over the documented range of the scalar type, ROUNDED to it (returned in it): the device and the oracle get
    the same numbers"""
    nd = np.dtype(dtype).type
    span = FAR_SPAN[nd]
    return _rng(9, n, rank, 4).uniform(-span, span, (n, nj)).astype(nd)


def far_batch(cfg, n, total_mass, dtype, rank=0):
    """wide_batch's attitude and position layers with far_joints as the joint angles; q, v in `dtype` (everything else float64, as make_batch)"""
    B = wide_batch(cfg, n, total_mass, rank, layers=("attitude", "position"))
    B["q"] = B["q"].astype(dtype)
    B["q"][:, 7:] = far_joints(n, dtype, rank)
    B["v"] = B["v"].astype(dtype)
    return B


def heading_norm2(q):
    """R00^2 + R10^2 of the base attitude, [N]"""
    R = SR._quat_R(np.asarray(q, np.float64)[:, 3:7])
    return R[:, 0, 0] ** 2 + R[:, 1, 0] ** 2


def heading_ok(q):
    """bool [N]: the states a gait case keeps; asserts the cap"""
    keep = heading_norm2(q) >= HEADING_MIN
    assert (~keep).mean() <= HEADING_SKIP_CAP, (~keep).mean()
    return keep


# ---- the quaternion step
def spin_batch(cfg, n, total_mass, rank=0, layers=LAYERS):
    """wide_batch with base angular velocities for dt = SPIN_DT: state i has theta = |omega| dt = 1.5 (i mod 16 + 1/2) / 16 about a random axis, so every
    16-state group spans 0.05 ... 1.45 rad with 5 states below the switch at 0.5 and 11 above.  Special states, where present: 1 and 2 have omega = 0
    exactly and an attitude whose squared norm is exactly 1 (1/2, 1/2, 1/2, 1/2 with signs), 3 and 4 have theta = 0.5 - 5e-4 and 0.5 + 5e-4.
    Returns the batch with B["dt"], B["theta"] [n] and B["quiet"] (indices of the special states: a test that wants their theta to survive the
    velocity update gives them zero acceleration)."""
    B = wide_batch(cfg, n, total_mass, rank, layers)
    rng = _rng(cfg, n, rank, 5)
    theta = SPIN_THETA_MAX * ((np.arange(n) % 16) + 0.5) / 16.0
    quiet = [i for i in (1, 2, 3, 4) if i < n]
    for i, th in zip((1, 2, 3, 4), (0.0, 0.0, SPIN_SWITCH - 5e-4, SPIN_SWITCH + 5e-4)):
        if i < n:
            theta[i] = th
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    B["v"][:, 3:6] = ax * (theta / SPIN_DT)[:, None]
    for i, sg in ((1, (1, 1, 1, 1)), (2, (-1, 1, -1, 1))):
        if i < n:
            B["v"][i, 3:6] = 0.0
            B["q"][i, 3:7] = 0.5 * np.array(sg, np.float64)
    B["dt"], B["theta"], B["quiet"] = SPIN_DT, theta, np.array(quiet, np.int64)
    return B


def integrate_ref(dt, M, h, Jc, tau, f, tau_ext, q, v):
    """wbc_integrate_batch in float64: vdot = M^-1 (S^T tau + Jc^T f + tau_ext - h) by numpy's LU on the unpacked M [N, nv, nv], then
    v += dt vdot and q <- q (+) dt v by crosscheck_np.integrate_q.  Returns (q', v'); the arguments are not modified."""
    M, h, Jc, tau, f, tau_ext, q, v = (np.asarray(a, np.float64) for a in (M, h, Jc, tau, f, tau_ext, q, v))
    N, nv = v.shape
    qn, vn = np.empty_like(q), np.empty_like(v)
    for s in range(N):
        rhs = tau_ext[s] - h[s] + Jc[s].reshape(-1, nv).T @ f[s]
        rhs[6:] += tau[s]
        vn[s] = v[s] + dt * np.linalg.solve(M[s], rhs)
        qn[s] = X.integrate_q(q[s], vn[s], dt)
    return qn, vn


# ---- swing and gait cases on wide states
def wide_swing_case(flat, total_mass, n, rank=0):
    """swing_ref.swing_case(n, rank) carried to the wide state of the same index: q from wide_batch (all layers), every foot's plan points p0, p1 moved
    by where that foot went, so that the plans still lie around the feet.  dict(q, v, mask, swing, vdot_des, t)"""
    c = SR.swing_case(flat, total_mass, n, rank=rank)
    q = wide_batch(3, n, total_mass, rank=70 + rank)["q"]
    swing = c["swing"].copy()
    for k in range(4):
        shift = SR.foot_kin(flat, k, q, c["v"])["pf"] - SR.foot_kin(flat, k, c["q"], c["v"])["pf"]
        swing[:, 9 * k:9 * k + 3] += shift
        swing[:, 9 * k + 3:9 * k + 6] += shift
    return dict(c, q=q, swing=swing)


def wide_branch_case(flat, total_mass, n, rank=0, P=None, dt_ctl=1e-3):
    """gait_ref.branch_case(n, rank) with q from wide_batch (all layers): the mask rule reads phase, mask and contact only, so the case still takes every
    branch for every foot.  dict(q, v, cmd, contact, phase, mask, swing, keep); keep = heading_ok(q)"""
    c = GR.branch_case(flat, total_mass, n, rank=rank, P=P, dt_ctl=dt_ctl)
    q = wide_batch(3, n, total_mass, rank=90 + rank)["q"]
    return dict(c, q=q, keep=heading_ok(q))


def wide_plan(B, rank=0):
    """synth.make_plan around the wide states, with desired attitudes uniform on the sphere (make_plan's edge rows kept)"""
    plan = synth.make_plan(B, rank=rank)
    n = plan.shape[0]
    qq = _rng(0, n, rank, 6).normal(size=(n, 4))
    plan[:, 8:12] = qq / np.linalg.norm(qq, axis=1, keepdims=True)
    return plan


def reference_case(n, total_mass):
    """(B, plan) of the reference-generator cases: wide config-4 states, plans around them with desired attitudes over the whole sphere"""
    B = wide_batch(4, n, total_mass, rank=n)
    return B, wide_plan(B, rank=n)


def f32_reference_errors(oracle, G, total_mass):
    """the measurement behind F32_REFERENCE: the fp32 oracle against the fp64 oracle"""
    worst = dict(w_des=0.0, vdot_des=0.0, com=0.0)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    for n in REFERENCE_SIZES:
        B, plan = reference_case(n, total_mass)
        r64, r32 = oracle.reference(G, B["q"], B["v"], plan, REFERENCE_T), oracle.reference(G, f(B["q"]), f(B["v"]), f(plan), REFERENCE_T)
        for k in worst:
            worst[k] = max(worst[k], float(np.abs(r32[k] - r64[k]).max() / np.abs(r64[k]).max()))
    return worst


def f32_swing_errors(flat, total_mass, sizes=SIZES):
    """the measurement behind F32_SWING: swing_ref in float32 against float64 on wide_swing_case(n, rank=n)"""
    worst = dict(vdot=0.0, foot=0.0)
    f = lambda a: a.astype(np.float32)
    for n in sizes:
        c = wide_swing_case(flat, total_mass, n, rank=n)
        vd64, ft64 = SR.swing_reference(flat, c["q"], c["v"], c["mask"], c["swing"], c["t"], c["vdot_des"])
        vd32, ft32 = SR.swing_reference(flat, f(c["q"]), f(c["v"]), c["mask"], f(c["swing"]), c["t"], f(c["vdot_des"]))
        w = np.zeros((n, 18), bool)
        for k, js in enumerate(limit_ref.leg_joints(flat)):
            for j in js:
                w[((c["mask"] >> k) & 1) == 0, 6 + j] = True
        if w.any():
            worst["vdot"] = max(worst["vdot"], float(np.abs(vd32[w] - vd64[w]).max() / np.abs(vd64[w]).max()))
        worst["foot"] = max(worst["foot"], float(np.abs(ft32 - ft64).max() / np.abs(ft64).max()))
    return worst


def f32_gait_errors(flat, total_mass, sizes=SIZES, dt_ctl=1e-3):
    """the measurement behind F32_GAIT: gait_ref.gait_tick in float32 against float64 on wide_branch_case(n, rank=n) (kept states); asserts on the way
    that float32 takes the same branches"""
    P = GR.params(flat)
    worst = dict(phase=0.0, p0=0.0, p1=0.0, t0=0.0)
    f = lambda a: a.astype(np.float32)
    for n in sizes:
        c = wide_branch_case(flat, total_mass, n, rank=n, P=P, dt_ctl=dt_ctl)
        kp = c["keep"]
        r64 = GR.gait_tick(flat, P, dt_ctl, c["q"], c["v"], c["cmd"], c["contact"], c["phase"], c["mask"], c["swing"])
        r32 = GR.gait_tick(flat, P, dt_ctl, f(c["q"]), f(c["v"]), f(c["cmd"]), c["contact"], f(c["phase"]), c["mask"], f(c["swing"]))
        assert np.array_equal(r32[1], r64[1]) and np.array_equal(r32[3], r64[3])
        p0, p1, t0, _ = GR.written_words(r64[1], r64[3])
        worst["phase"] = max(worst["phase"], float(np.abs(r32[0] - r64[0])[kp].max() / np.abs(r64[0])[kp].max()))
        for what, w in (("p0", p0), ("p1", p1), ("t0", t0)):
            w = w & kp[:, None]
            if w.any():
                worst[what] = max(worst[what], float(np.abs(r32[2][w] - r64[2][w]).max() / np.abs(r64[2][w]).max()))
    return worst


# ---- rollouts
def rollout_inputs(oracle, B, obs, nd):
    """(P, tau_ext, integ, r) of a rollout from the batch B (wide_batch / spin_batch) in the scalar type nd: B's own dt, the batch's pushes on the base
    as tau_ext, the observer started at integ = M v, r = 0"""
    n = B["q"].shape[0]
    P = synth.default_params(observer_order=obs, dtype="f64" if nd == np.float64 else "f32")
    P["dt"] = B.get("dt", P["dt"])
    tau_ext = np.zeros((n, 18), nd)
    tau_ext[:, 0:3] = B["push"]
    integ = np.ascontiguousarray(oracle.dynamics(B["q"], B["v"], nthreads=8)["p"], nd) if obs else None
    r = np.zeros((n, 18), nd) if obs else None
    return P, tau_ext, integ, r


def oracle_rollout(oracle, B, H, obs, nd, plan=None, G=None):
    """oracle.rollout (plan given: oracle.rollout_tracking with the gains G) of H ticks in the scalar type nd.
    dict(q, v, status, tau_traj [n, H, 12][, integ, r])"""
    c = lambda a: np.ascontiguousarray(a, nd)
    P, tau_ext, integ, r = rollout_inputs(oracle, B, obs, nd)
    q, v = c(B["q"]).copy(), c(B["v"]).copy()
    if plan is None:
        o = oracle.rollout(P, H, q, v, c(B["w_des"]), c(B["vdot_des"]), c(B["normals"]), c(B["mu"]), B["mask"], tau_ext=tau_ext, integ=integ, r=r,
                           want_traj=True, nthreads=8)
    else:
        o = oracle.rollout_tracking(P, G, H, q, v, c(plan), c(B["normals"]), c(B["mu"]), B["mask"], tau_ext=tau_ext, integ=integ, r=r, want_traj=True,
                                    nthreads=8)
    out = dict(q=q, v=v, status=o["status"], tau_traj=o["tau_traj"])
    if obs:
        out["integ"], out["r"] = integ, r
    return out
