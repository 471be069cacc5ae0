"""Plant payload (wbc_*_plant_batch) restated in numpy, for the tests (test infrastructure).

A payload = a rigid body fixed to the trunk (body 0): m, c (CoM in the base frame), I (about c, base axes).  Two independent routes:
  merge_payload: the trunk link of a flat model with the payload folded in (parallel-axis rule), for oracle.Oracle(merged).dynamics;
  delta_terms:   the closed form of what it adds to the base block of M and the base rows of h (include/wbc_hip.h).
plant_step: one step of the plant (merged model's M, h; np.linalg.solve; the oracle's semi-implicit Euler, oracle/wbc_oracle.hpp
integrate_state, restated).
"""
import copy

import numpy as np

PAYLOAD_WORDS = 10


def _sym6_to_mat(w):
    """xx yy zz xy xz yz -> 3x3"""
    xx, yy, zz, xy, xz, yz = w
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def _ic_to_mat(w):
    """flat model Ic row (xx xy xz yy yz zz, oracle/wbc_oracle.hpp model_from_flat) -> 3x3"""
    xx, xy, xz, yy, yz, zz = w
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def unpack(payload_row):
    """one state's payload words -> (m, c [3], I [3, 3])"""
    p = np.asarray(payload_row, np.float64)
    return p[0], p[1:4].copy(), _sym6_to_mat(p[4:10])


def random_payloads(rng, n, m_max=8.0, c_max=0.15, zero_every=5):
    """[n, 10] mixed payloads: 0 .. m_max kg, CoM offsets within c_max m per axis, a random PSD inertia of a compact body, and every
    `zero_every`-th row all zeros (no payload)"""
    out = np.zeros((n, PAYLOAD_WORDS))
    for i in range(n):
        if zero_every and i % zero_every == 0:
            continue
        m = rng.uniform(0.0, m_max)
        A = rng.normal(size=(3, 3))
        Q, _ = np.linalg.qr(A)
        d = rng.uniform(0.2, 1.0, 3) * m * 0.01   # principal moments of a body ~0.1-0.3 m across
        I = Q @ np.diag(d) @ Q.T
        out[i] = [m, *rng.uniform(-c_max, c_max, 3), I[0, 0], I[1, 1], I[2, 2], I[0, 1], I[0, 2], I[1, 2]]
    return out


def merge_payload(flat, m, c, I):
    """A copy of the flat model whose trunk link also carries the payload (m, c, I about c)."""
    f = copy.deepcopy(flat)
    for k in ("mass", "com", "Ic"):
        f[k] = np.array(flat[k], dtype=np.float64, copy=True)
    m0, c0, I0 = float(f["mass"][0]), f["com"][0].copy(), _ic_to_mat(f["Ic"][0])
    mt = m0 + m
    ct = (m0 * c0 + m * np.asarray(c)) / mt
    shift = lambda mm, d: mm * (np.dot(d, d) * np.eye(3) - np.outer(d, d))
    It = I0 + shift(m0, c0 - ct) + np.asarray(I) + shift(m, np.asarray(c) - ct)
    f["mass"][0] = mt
    f["com"][0] = ct
    f["Ic"][0] = [It[0, 0], It[0, 1], It[0, 2], It[1, 1], It[1, 2], It[2, 2]]
    return f


def quat_R(qx, qy, qz, qw):
    n = np.sqrt(qx * qx + qy * qy + qz * qz + qw * qw)
    x, y, z, w = qx / n, qy / n, qz / n, qw / n
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def delta_terms(q, v, payload, g):
    """(dM [6, 6], dh [6]) of one state: what the payload adds to the base block of M and to the base rows of h"""
    m, c, I = unpack(payload)
    R = quat_R(*q[3:7])
    r = R @ c
    Iw = R @ I @ R.T
    om = np.asarray(v[3:6], np.float64)
    rx = _skew(r)
    dM = np.zeros((6, 6))
    dM[:3, :3] = m * np.eye(3)
    dM[:3, 3:] = -m * rx
    dM[3:, :3] = m * rx
    dM[3:, 3:] = Iw - m * rx @ rx
    f = m * np.cross(om, np.cross(om, r)) - m * np.asarray(g)
    dh = np.concatenate([f, np.cross(r, f) + np.cross(om, Iw @ om)])
    return dM, dh


def integrate_state(q, v, vdot, dt):
    """oracle/wbc_oracle.hpp integrate_state: semi-implicit Euler, the base attitude by the left-multiplied increment"""
    q, v = np.array(q, np.float64), np.array(v, np.float64)
    v = v + dt * vdot
    q[0:3] += dt * v[0:3]
    w = v[3:6] * dt
    th = np.sqrt(w @ w)
    if th > 1e-8:
        sc, cw = np.sin(th / 2) / th, np.cos(th / 2)
    else:
        sc, cw = 0.5 - th * th / 48, 1 - th * th / 8
    dx, dy, dz = sc * w
    x, y, z, ww = q[3:7] / np.linalg.norm(q[3:7])
    q[3:7] = [cw * x + dx * ww + dy * z - dz * y, cw * y - dx * z + dy * ww + dz * x, cw * z + dx * y - dy * x + dz * ww,
              cw * ww - dx * x - dy * y - dz * z]
    q[7:] += dt * v[6:]
    return q, v


def plant_step(merged_oracle, q, v, tau, f, dt, tau_ext=None, nf=4):
    """One plant step of ONE state: M_p, h_p, Jc of the merged model (oracle.dynamics), vdot = M_p^-1 (S^T tau + Jc^T f + tau_ext - h_p),
    then integrate_state.  q [19], v [18], tau [12], f [3 nf] -> (q', v')"""
    from tests.util import unpack_M
    nv = v.shape[0]
    d = merged_oracle.dynamics(q[None, :].astype(np.float64), v[None, :].astype(np.float64))
    Mp = unpack_M(d["M"][0], nv)
    Jc = d["Jc"][0].reshape(3 * nf, nv)
    rhs = Jc.T @ f - d["h"][0]
    rhs[6:] += tau
    if tau_ext is not None:
        rhs = rhs + tau_ext
    vdot = np.linalg.solve(Mp, rhs)
    return integrate_state(q, v, vdot, dt)


class MergedOracles:
    """One oracle per distinct payload row (rows of zeros share the nominal one)"""

    def __init__(self, flat, payloads):
        from oracle import oracle_py
        self.nominal = oracle_py.Oracle(flat)
        self.per_state = []
        for p in payloads:
            if not np.any(p):
                self.per_state.append(self.nominal)
            else:
                m, c, I = unpack(p)
                self.per_state.append(oracle_py.Oracle(merge_payload(flat, m, c, I)))

    def step(self, q, v, tau, f, dt, tau_ext=None):
        """plant_step of every state: q [n, 19], v [n, 18], tau [n, 12], f [n, 12]"""
        qn, vn = np.empty_like(q, dtype=np.float64), np.empty_like(v, dtype=np.float64)
        for i, orc in enumerate(self.per_state):
            qn[i], vn[i] = plant_step(orc, q[i], v[i], tau[i], f[i], dt, None if tau_ext is None else tau_ext[i])
        return qn, vn
