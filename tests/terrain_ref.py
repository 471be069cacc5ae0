"""Terrain heightfield (wbc_terrain_sample_batch, wbc_terrain_feet_batch, wbc_gait[_estimated]_terrain_batch; include/wbc_hip.h "Terrain heightfield")
restated in numpy, for the tests (test infrastructure).

A terrain is a dict(z [n_tiles, ny, nx] float64, x0, y0, cell).  Row-per-state arrays in the dtype of the inputs, like tests/gait_ref.py.
  consts        inv_cell, x_max, y_max, x0, y0 as the host forms them: in double, rounded to the scalar type
  sample        the law at points, in the header's operation order: dict(z, n [M, 3], d, gx, gy, ix, iy)
  edge_margin   the smallest distance of gx, gy from an integer (the normal jumps there)
  feet          the planes under the four feet, and p1_z of the lifted feet's plans
  grid_plane / grid_ripple / parity_grid / walk_grids / fit_grid; branch_case / feet_case   grids and cases
  walk_case / closed_loop / cpu_walk   the walking loop on a terrain: gait_tick -> feet -> oracle.reference -> swing_reference -> oracle.step ->
                stick_ref.integrate_ground_stick.  tests/walk_ref.py's loop has one fixed set of normals; here the planes change every tick and the
                controller's may differ from the plant's (aware / blind), so this loop is its own.
"""
import numpy as np

from tests import gait_ref as GR, ground_ref, limit_ref, stick_ref, swing_ref as SR, walk_ref
from wbc_quadruped_dob_amd import synth

MARGIN64, MARGIN32 = 1e-6, 1e-3     # cells: how far from a cell edge a parity point must stay in float64 / float32 terms


def consts(T, dtype):
    t = np.dtype(dtype).type
    nz, ny, nx = T["z"].shape
    return dict(x0=t(T["x0"]), y0=t(T["y0"]), inv=t(1.0 / T["cell"]), x_max=t(T["x0"] + (nx - 1) * T["cell"]), y_max=t(T["y0"] + (ny - 1) * T["cell"]))


def sample(T, x, y, tile=None):
    """The law at the points (x [M], y [M]) on the tiles tile [M] (None: tile 0), arithmetic in x's dtype.  cx, cy: the coordinate was clamped."""
    dt = x.dtype
    t = dt.type
    y = np.asarray(y, dt)
    z = T["z"].astype(dt)
    nz, ny, nx = z.shape
    c = consts(T, dt)
    tile = np.zeros(x.shape, np.int64) if tile is None else np.asarray(tile, np.int64)
    xc = np.minimum(np.maximum(x, c["x0"]), c["x_max"])
    yc = np.minimum(np.maximum(y, c["y0"]), c["y_max"])
    gx = ((xc - c["x0"]) * c["inv"]).astype(dt)
    gy = ((yc - c["y0"]) * c["inv"]).astype(dt)
    ix = np.minimum(gx.astype(np.int64), nx - 2)
    iy = np.minimum(gy.astype(np.int64), ny - 2)
    u, w = (gx - ix.astype(dt)).astype(dt), (gy - iy.astype(dt)).astype(dt)
    z00, z10, z01, z11 = z[tile, iy, ix], z[tile, iy, ix + 1], z[tile, iy + 1, ix], z[tile, iy + 1, ix + 1]
    a = z00 + u * (z10 - z00)
    b = z01 + u * (z11 - z01)
    zs = a + w * (b - a)
    zx = ((z10 - z00) + w * ((z11 - z01) - (z10 - z00))) * c["inv"]
    zy = (b - a) * c["inv"]
    r = t(1) / np.sqrt(zx * zx + zy * zy + t(1))
    n = np.stack([-zx * r, -zy * r, r], 1).astype(dt)
    d = n[:, 0] * xc + n[:, 1] * yc + n[:, 2] * zs
    return dict(z=zs.astype(dt), n=n, d=d.astype(dt), gx=gx, gy=gy, ix=ix, iy=iy, u=u, w=w, cx=xc != x, cy=yc != y)


def edge_margin(s):
    """smallest |g - round(g)| over gx, gy of a sample() result, in cells (float64 arithmetic).  Clamped coordinates do not count: beyond an edge the
    cell is the edge's whatever the rounding, and zs, n, d are continuous there."""
    g = np.concatenate([np.asarray(s["gx"], np.float64)[~s["cx"]], np.asarray(s["gy"], np.float64)[~s["cy"]]])
    return float(np.abs(g - np.round(g)).min()) if g.size else np.inf


def inside(T, x, y):
    nz, ny, nx = T["z"].shape
    return bool(np.all((x >= T["x0"]) & (x <= T["x0"] + (nx - 1) * T["cell"]) & (y >= T["y0"]) & (y <= T["y0"] + (ny - 1) * T["cell"])))


def feet(flat, T, q, mask=None, swing=None, tile=None):
    """-> dict(normals [N, 12], height [N, 4], surf [N, 4], pf [N, 4, 3], swing: a copy with p1_z of every foot whose mask bit is clear := zs at its
    plan's own p1_x, p1_y (None without mask), margin: edge_margin over every sample taken, inside: every sampled point lies on the grid)"""
    dt = q.dtype
    N = q.shape[0]
    v0 = np.zeros((N, q.shape[1] - 1), dt)
    out = dict(normals=np.zeros((N, 12), dt), height=np.zeros((N, 4), dt), surf=np.zeros((N, 4), dt), pf=np.zeros((N, 4, 3), dt),
               swing=None if mask is None else np.array(swing, dt), margin=np.inf, inside=True)
    for k in range(4):
        pf = SR.foot_kin(flat, k, q, v0)["pf"]
        s = sample(T, np.ascontiguousarray(pf[:, 0]), np.ascontiguousarray(pf[:, 1]), tile)
        out["normals"][:, 3 * k:3 * k + 3], out["height"][:, k], out["surf"][:, k], out["pf"][:, k] = s["n"], s["d"], s["z"], pf
        out["margin"] = min(out["margin"], edge_margin(s))
        out["inside"] = out["inside"] and inside(T, pf[:, 0], pf[:, 1])
        if mask is not None:
            air = ((np.asarray(mask) >> k) & 1) == 0
            if air.any():
                sw = out["swing"]
                x, y = np.ascontiguousarray(sw[air, 9 * k + 3]), np.ascontiguousarray(sw[air, 9 * k + 4])
                s1 = sample(T, x, y, None if tile is None else np.asarray(tile)[air])
                sw[air, 9 * k + 5] = s1["z"]
                out["margin"] = min(out["margin"], edge_margin(s1))
                out["inside"] = out["inside"] and inside(T, x, y)
    return out


# ---- grids
def grid_plane(nx, ny, x0, y0, cell, c, a, b, n_tiles=1):
    """nodes of z = c + a x + b y (tile t: c + t / 8), float64"""
    X, Y = np.meshgrid(x0 + cell * np.arange(nx), y0 + cell * np.arange(ny))
    return dict(z=np.stack([c + t / 8.0 + a * X + b * Y for t in range(n_tiles)]), x0=x0, y0=y0, cell=cell)


def grid_ripple(nx, ny, x0, y0, cell, z0, slope, amp, lx, ly, n_tiles=1):
    """tile t: z0 + slope x + amp sin(2 pi (x / lx + t / 4)) cos(2 pi y / ly)"""
    X, Y = np.meshgrid(x0 + cell * np.arange(nx), y0 + cell * np.arange(ny))
    return dict(z=np.stack([z0 + slope * X + amp * np.sin(2 * np.pi * (X / lx + t / 4.0)) * np.cos(2 * np.pi * Y / ly) for t in range(n_tiles)]),
                x0=x0, y0=y0, cell=cell)


PARITY_GRIDS = ("2x2", "3x2", "64x48", "64x48x4")


def parity_grid(name):
    """the grids of the device parity tests: the minimal grid, one with a last cell that is not the first, the walking loop's size with 1 and 4 tiles.
    Origins and cells are dyadic, so that points built as x0 + (i + dyadic fraction) cell are exact."""
    rng = np.random.default_rng(synth.SEED + 1500)
    if name == "2x2":
        return dict(z=np.array([[[0.25, 0.5], [0.375, 0.125]]]), x0=-0.5, y0=-0.25, cell=1.0)
    if name == "3x2":
        return dict(z=rng.uniform(-0.1, 0.1, (1, 2, 3)), x0=-0.25, y0=0.5, cell=0.25)
    nt = 4 if name == "64x48x4" else 1
    T = grid_ripple(64, 48, -0.5, -0.375, 2.0 ** -6, 0.1, 0.05, 0.006, 0.125, 0.25, nt)
    return T


def branch_case(T, m, rank=0):
    """m points (x, y, tile) that between them -- for m >= 15 -- take every branch of the law: interior cells, beyond each edge and each corner, the
    last cell (ix = nx - 2, iy = ny - 2), exact nodes (the last row and column among them) and, with several tiles, every tile.  Interior
    and last-cell points are x0 + (i + f) cell with f a multiple of 1/8 in [1/8, 7/8]: exact in float32 and float64, 1/8 of a cell clear of every edge.
    dict(x, y, tile, node: bool [m] the point is a node, node0: it is one with u = w = 0, where zs is the node's own bits)"""
    nz, ny, nx = T["z"].shape
    rng = np.random.default_rng(synth.SEED + 1510 + rank)
    x0, y0, c = T["x0"], T["y0"], T["cell"]
    ci = rng.integers(0, nx - 1, m); cj = rng.integers(0, ny - 1, m)
    fx = rng.integers(1, 8, m) / 8.0; fy = rng.integers(1, 8, m) / 8.0
    x = x0 + (ci + fx) * c
    y = y0 + (cj + fy) * c
    node, node0 = np.zeros(m, bool), np.zeros(m, bool)
    xm, ym = x0 + (nx - 1) * c, y0 + (ny - 1) * c
    special = [(x0 - 0.3, None), (xm + 0.3, None), (None, y0 - 0.3), (None, ym + 0.3),                       # beyond each edge
               (x0 - 0.2, y0 - 0.1), (xm + 0.2, y0 - 0.1), (x0 - 0.2, ym + 0.1), (xm + 0.2, ym + 0.1),       # beyond each corner
               (x0 + (nx - 2 + 0.5) * c, y0 + (ny - 2 + 0.25) * c),                                          # the last cell
               ("node", (0, 0)), ("node", (nx - 1, ny - 1)), ("node", (nx - 1, 0)), ("node", (0, ny - 1)), ("node", ((nx - 1) // 2, (ny - 1) // 2))]
    for i, (a, b) in enumerate(special):
        j = m - 1 - i       # from the end, so that the first point of every case is an interior one
        if j < 1:
            break
        if a == "node":
            x[j], y[j], node[j], node0[j] = x0 + b[0] * c, y0 + b[1] * c, True, b[0] < nx - 1 and b[1] < ny - 1
        else:
            if a is not None:
                x[j] = a
            if b is not None:
                y[j] = b
    tile = (np.arange(m) % nz).astype(np.int32)
    return dict(x=x, y=y, tile=tile, node=node, node0=node0)


FEET_SIZES = GR.PARITY_SIZES


def fit_grid(flat, q, mask=None, swing=None, tile=None, nx=64, ny=48):
    """The rippled 64 x 48 x 4 grid (cell 2^-6; nx, ny: another size) moved under a batch: its origin is the batch's mean foot position minus half the
    grid, rounded to 1/16 of a cell, then shifted by the first of j / 16 cells, j = 0 .. 15 (x and y alike), at which every sample feet() takes keeps
    MARGIN64 / MARGIN32 clear of a cell edge in float64 / float32.  -> (T, feet() in float64, feet() in float32)"""
    n = q.shape[0]
    pf = np.stack([SR.foot_kin(flat, k, q, np.zeros((n, q.shape[1] - 1)))["pf"] for k in range(4)], 1)
    cell = 2.0 ** -6
    ox, oy = (np.round((pf[:, :, i].mean() - 0.5 * (m - 1) * cell) / cell * 16) / 16 * cell for i, m in ((0, nx), (1, ny)))
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
    for j in range(16):
        T = grid_ripple(nx, ny, ox + j * cell / 16, oy + j * cell / 16, cell, 0.1, 0.05, 0.006, 0.125, 0.25, 4)
        F64, F32 = feet(flat, T, q, mask, swing, tile), feet(flat, T, f32(q), mask, f32(swing), tile)
        if F64["margin"] >= MARGIN64 and F32["margin"] >= MARGIN32:
            return T, F64, F32
    raise AssertionError("no grid offset keeps the case clear of the cell edges")


def feet_case(flat, total_mass, n, rank=0, q=None, nx=64, ny=48):
    """gait_ref.branch_case states (q: these instead -- tests/walk_edges.py) with every mask pattern (swing_ref.all_masks), plans whose p1_x, p1_y lie
    within 5 cm of the foot (the other swing words stay recognisable junk), tile i mod 4, and fit_grid's terrain (of nx x ny nodes).
    dict(q, mask, swing, tile, T, ref64, ref32)"""
    c = GR.branch_case(flat, total_mass, n, rank=rank)
    rng = np.random.default_rng(synth.SEED + 1520 + rank)
    q, swing = c["q"] if q is None else q, c["swing"].copy()
    for k in range(4):
        swing[:, 9 * k + 3:9 * k + 5] = SR.foot_kin(flat, k, q, np.zeros((n, 18)))["pf"][:, :2] + rng.uniform(-0.05, 0.05, (n, 2))
    mask, tile = SR.all_masks(n), (np.arange(n) % 4).astype(np.int32)
    T, F64, F32 = fit_grid(flat, q, mask, swing, tile, nx, ny)
    return dict(q=q, mask=mask, swing=swing, tile=tile, T=T, ref64=F64, ref32=F32)


# ---- the walking loop on a terrain
WALK_N, WALK_TICKS = 4, GR.WALK_TICKS
WALK_KT = stick_ref.DEFAULT_KT


def walk_case(flat, oracle, n=WALK_N):
    """gait_ref.walk_case + z0 = the mean starting foot height + m g / (4 k_n) (the feet start near the equilibrium penetration of flat ground) and
    tile [n] = robot i walks on tile i mod 4"""
    c = GR.walk_case(flat, oracle, n)
    pfz = np.stack([SR.foot_kin(flat, k, c["q"], c["v"])["pf"][:, 2] for k in range(4)], 1)
    P = ground_ref.params()
    c["z0"] = float(pfz.mean()) + float(np.sum(flat["mass"])) * float(np.linalg.norm(flat["gravity"])) / (4 * P["k_n"])
    c["tile"] = (np.arange(n) % 4).astype(np.int32)
    return c


def walk_grids(z0):
    """the two terrains of the walking-loop tests: flat ground and the four rippled ramps (64 x 48 nodes, cell 2^-6, origin (-0.5, -0.375))"""
    flat_T = grid_ripple(64, 48, -0.5, -0.375, 2.0 ** -6, z0, 0.0, 0.0, 0.125, 0.25, 4)
    tiles = grid_ripple(64, 48, -0.5, -0.375, 2.0 ** -6, z0, 0.05, 0.006, 0.125, 0.25, 4)
    return dict(flat=flat_T, tiles=tiles)


def closed_loop(flat, oracle, case, T, aware=True, ticks=WALK_TICKS, k_t=WALK_KT, q0=None):
    """Per tick: gait_tick(contact = the plant's last word, p1_z = cmd row 3) -> feet(T, q, mask, swing) -> oracle.reference -> swing_reference ->
    oracle.step -> stick_ref.integrate_ground_stick.  The plant always stands on the terrain's planes under the feet.
    aware: the swing plans' p1_z and the controller's normals are feet()'s, as wbc_gait_terrain_batch leaves them.  Not aware: p1_z = z_g and the
    controller's normals are the case's (e_z): what the calls without a terrain can do.
    Returns dict(q, v at the end; masks, events, contacts [ticks, N]; status_ok; touchdowns: list of (tick, state, foot, gap) with gap =
    p_f,z - zs(p_f,xy) at the tick of the foot's touchdown event; gap_max: the largest |gap|; gap_range; fn_max; margin: the smallest cell-edge distance
    of any sample taken (cells); inside: every sampled point lay on the grid)"""
    prm, G, GP, P = synth.default_params(observer_order=0), SR.loop_ref_params(), GR.walk_params(flat), ground_ref.params()
    prm["dt"] = GR.DYADIC_DT
    legs = limit_ref.leg_joints(flat)
    q, v = (case["q"] if q0 is None else q0).copy(), case["v"].copy()
    n = q.shape[0]
    phase, mask, swing = case["phase"].copy(), case["mask"].copy(), case["swing"].copy()
    contact, anchor, stick = np.zeros(n, np.int32), np.zeros((n, 12)), np.zeros(n, np.int32)
    rec = dict(masks=[], events=[], contacts=[])
    ok, margin, ins, fn_max, touchdowns = True, np.inf, True, 0.0, []
    for k in range(ticks):
        phase, mask, swing, ev = GR.gait_tick(flat, GP, prm["dt"], q, v, case["cmd"], contact, phase, mask, swing)
        F = feet(flat, T, q, mask, swing, case["tile"])
        margin, ins = min(margin, F["margin"]), ins and F["inside"]
        if aware:
            swing = F["swing"]
        normals = F["normals"] if aware else case["normals"]
        for f in range(4):
            for s in np.nonzero((ev >> (4 + f)) & 1)[0]:
                touchdowns.append((k, int(s), f, float(F["pf"][s, f, 2] - F["surf"][s, f])))
        ref = oracle.reference(G, q, v, case["plan"], k * prm["dt"])
        vd, _ = SR.swing_reference(flat, q, v, mask, swing, 0.0, ref["vdot_des"], GR.WALK_SWING_PARAMS)
        tick = oracle.step(prm, q, v, ref["w_des"], vd, normals, case["mu"], mask, None, None, None, None)
        ok = ok and bool(np.all(tick["status"] == 0))
        dyn = oracle.dynamics(q, v)
        q, v, g = stick_ref.integrate_ground_stick(P, k_t, prm["dt"], dyn, tick["tau"], F["normals"], F["height"], case["mu"], None, q, v, anchor, stick,
                                                   legs)
        anchor, stick, contact = g["anchor"], g["stick"], g["contact"]
        fn_max = max(fn_max, float(g["fn"].max()))
        rec["masks"].append(mask.copy()); rec["events"].append(ev.copy()); rec["contacts"].append(contact.copy())
    gaps = np.array([t[3] for t in touchdowns])
    out = dict(q=q, v=v, status_ok=ok, touchdowns=touchdowns, gap_max=float(np.abs(gaps).max()), gap_range=(float(gaps.min()), float(gaps.max())),
               fn_max=fn_max, margin=margin, inside=ins)
    out.update({key: np.array(val) for key, val in rec.items()})
    return out


def cpu_walk(flat, oracle, terrain="tiles", aware=True):
    """(case with case["T"] = the terrain, closed_loop(case)) of WALK_N robots, computed once per process and shared by the tests that need it: read only"""
    def make():
        c = walk_case(flat, oracle)
        c["T"] = walk_grids(c["z0"])[terrain]
        return c
    return walk_ref.cached(("terrain", id(flat), terrain, bool(aware)), make, lambda case: closed_loop(flat, oracle, case, case["T"], aware))


# amplification of a 1e-12 relative perturbation of q0 over the aware walking loop on the tiles, measured by tests/test_terrain_oracle.py (2.7), rounded
# up: the device loop's gate in tests/test_gpu_terrain.py is max(1e-6, 10 A 1e-9), the rule of tests/test_gpu_ground.py
WALK_AMPLIFICATION = 3.0
