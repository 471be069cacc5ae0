"""The cost of the scored rollouts and the per-group selection, restated in numpy float64 from the definition in include/wbc_hip.h
(wbc_rollout_scored_batch) -- the reference the GPU tests compare against.  Arrays are row-per-state ([N, c]), as the oracle's.

W: dict with the wbc_score_params fields (missing keys: the defaults -- every weight 0, w_fail = 1e6, terminal = 1, q_nom = 0).
goal [N, 10]: g_p (3), g_quat (x, y, z, w), g_v (3)."""
import numpy as np

DEFAULTS = dict(w_tau=0.0, w_f=0.0, w_fail=1e6, w_pos=0.0, w_rot=0.0, w_vel=0.0, w_omega=0.0, w_q=0.0, w_qd=0.0, terminal=1.0, q_nom=0.0)


def weights(W=None):
    out = dict(DEFAULTS)
    out.update(W or {})
    for k in ("w_pos", "w_rot", "w_vel", "w_omega"):
        out[k] = np.broadcast_to(np.asarray(out[k], np.float64), (3,))
    return out


def quat_mul(a, b):
    """Hamilton product of quaternions stored (x, y, z, w), row-wise"""
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def attitude_error(quat, quat_des):
    """e_R = 2 vec(quat_des (x) quat^-1), taken with a non-negative scalar part (wbc_reference_batch); inputs need not be normalised"""
    q = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
    d = quat_des / np.linalg.norm(quat_des, axis=-1, keepdims=True)
    e = quat_mul(d, q * np.array([-1.0, -1.0, -1.0, 1.0]))
    return 2.0 * np.where(e[..., 3:4] < 0, -1.0, 1.0) * e[..., :3]


def stage_cost(q, v, tau, f, status, goal, W=None, is_last=False):
    """l_k of every state: q [N, 19], v [N, 18] = the state the tick ENDED in; tau [N, 12], f [N, 12], status [N] = what it produced"""
    w = weights(W)
    q, v, tau, f, goal = (np.asarray(a, np.float64) for a in (q, v, tau, f, goal))
    nj = tau.shape[1]
    qn = np.asarray(w["q_nom"], np.float64).ravel()
    q_nom = np.broadcast_to(qn[:nj] if qn.size > 1 else qn, (nj,))
    l = w["w_tau"] * (tau ** 2).sum(1) + w["w_f"] * (f ** 2).sum(1) + w["w_fail"] * (np.asarray(status) != 0)
    e = attitude_error(q[:, 3:7], goal[:, 3:7])
    st = ((q[:, 0:3] - goal[:, 0:3]) ** 2 @ w["w_pos"] + e ** 2 @ w["w_rot"] + (v[:, 0:3] - goal[:, 7:10]) ** 2 @ w["w_vel"]
          + v[:, 3:6] ** 2 @ w["w_omega"] + w["w_q"] * ((q[:, 7:7 + nj] - q_nom) ** 2).sum(1) + w["w_qd"] * (v[:, 6:6 + nj] ** 2).sum(1))
    return l + (w["terminal"] if is_last else 1.0) * st


def rollout_cost(qs, vs, taus, fs, statuses, goal, W=None, cost_in=None, fail_in=None, terminal_last=True):
    """Sums stage_cost over a state path: qs[k], vs[k] = the state tick k ended in, taus[k], fs[k], statuses[k] = its outputs.
    terminal_last False: the last tick counts with s_k = 1 (a horizon that a later call continues).  Returns (cost [N], fail_ticks [N])."""
    H = len(qs)
    cost = np.zeros(len(qs[0])) if cost_in is None else np.asarray(cost_in, np.float64).copy()
    fail = np.zeros(len(qs[0]), np.int64) if fail_in is None else np.asarray(fail_in, np.int64).copy()
    Wl = dict(W or {})
    if not terminal_last:
        Wl["terminal"] = 1.0
    for k in range(H):
        cost += stage_cost(qs[k], vs[k], taus[k], fs[k], statuses[k], goal, Wl, is_last=(k == H - 1))
        fail += np.asarray(statuses[k]) != 0
    return cost, fail


def select(cost, group, lam=0.0):
    """Per group of `group` consecutive costs: best (index within the group of the smallest cost; ties: the lowest index; NaN counts as
    +inf; nothing finite: -1), best_cost, weights [N] = exp(-(c - c_min) / lam) normalised per group (lam <= 0: one-hot on best; a group
    with best = -1: zeros)."""
    c = np.asarray(cost, np.float64).reshape(-1, group).copy()
    c[np.isnan(c)] = np.inf
    best = np.argmin(c, axis=1).astype(np.int64)      # (numpy: the first occurrence of the minimum)
    cmin = c[np.arange(len(c)), best]
    none = ~(cmin < np.inf)
    best[none] = -1
    w = np.zeros_like(c)
    for g in range(len(c)):
        if none[g]:
            continue
        if lam > 0:
            with np.errstate(invalid="ignore"):
                e = np.exp(-(c[g] - cmin[g]) / lam)
            w[g] = e / e.sum()
        else:
            w[g, best[g]] = 1.0
    return best, cmin, w.reshape(-1)
