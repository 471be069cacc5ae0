"""Foothold selection (wbc_terrain_cost_batch, wbc_foothold_select_batch, wbc_gait[_estimated]_terrain_select_batch; include/wbc_hip.h "Foothold
selection") restated in numpy, for the tests (test infrastructure).

Terrains are tests/terrain_ref.py's dicts; row-per-state arrays in the dtype of the inputs.  No product is contracted on the device (foothold.hip.hpp),
so cost and J here are the device's own roundings in both scalar types.
  params        the library's defaults as a dict (overridable)
  cost_map      cost [n_tiles, ny, nx] of a terrain, vectorised; `step` and `slope2` beside it
  select        the law on (mask, swing, hold, latch) -> new swing, hold, latch and, per examined foot, what was decided and by what margin
  cost_grid     the grids of the cost-map tests
  ridges / ridge_grids / costly_nodes   the test terrains: flat ground with 2 cm ridges along y, and the nodes whose 3 x 3 neighbourhood holds a step
  branch_case   states that between them take every branch of the law
  closed_loop / cpu_walk   terrain_ref.closed_loop with select() between the gait rule and feet()
"""
import numpy as np

from tests import gait_ref as GR, ground_ref, limit_ref, stick_ref, swing_ref as SR, terrain_ref as TR, walk_ref
from wbc_quadruped_dob_amd import synth

DEFAULTS = dict(radius=3, margin=1, w_step=1.0, w_slope=2.0 ** -7, w_dist=4.0, cost_ok=0.00875, u_max=0.75)
MARGIN = 1e-3          # the smallest relative decision margin a parity case may have (the issue's figure)


def params(**kw):
    assert set(kw) <= set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


def cost_map(T, P, dtype=np.float64):
    """-> dict(cost, step, slope2), each [n_tiles, ny, nx] in dtype, in the header's operation order"""
    t = np.dtype(dtype).type
    z = T["z"].astype(dtype)
    nz, ny, nx = z.shape
    inv = TR.consts(T, dtype)["inv"]
    m = int(P["margin"])
    step = np.zeros_like(z)
    IX, IY = np.arange(nx), np.arange(ny)
    for dy in range(-m, m + 1):
        for dx in range(-m, m + 1):
            zz = z[:, np.clip(IY + dy, 0, ny - 1)][:, :, np.clip(IX + dx, 0, nx - 1)]
            step = np.maximum(step, np.abs(zz - z))
    fx = np.where((IX == 0) | (IX == nx - 1), t(1), t(0.5)).astype(dtype)
    fy = np.where((IY == 0) | (IY == ny - 1), t(1), t(0.5)).astype(dtype)
    sx = (z[:, :, np.clip(IX + 1, 0, nx - 1)] - z[:, :, np.clip(IX - 1, 0, nx - 1)]) * inv * fx[None, None, :]
    sy = (z[:, np.clip(IY + 1, 0, ny - 1)] - z[:, np.clip(IY - 1, 0, ny - 1)]) * inv * fy[None, :, None]
    slope2 = sx * sx + sy * sy
    cost = t(P["w_step"]) * step + t(P["w_slope"]) * slope2
    assert cost.dtype == np.dtype(dtype)
    return dict(cost=cost, step=step, slope2=slope2)


def nearest_node(T, x, y, dtype):
    """(jx, jy) of the law, arithmetic in dtype"""
    t = np.dtype(dtype).type
    c = TR.consts(T, dtype)
    nz, ny, nx = T["z"].shape
    jx = np.clip(np.floor((np.asarray(x, dtype) - c["x0"]) * c["inv"] + t(0.5)), 0, nx - 1).astype(np.int64)
    jy = np.clip(np.floor((np.asarray(y, dtype) - c["y0"]) * c["inv"] + t(0.5)), 0, ny - 1).astype(np.int64)
    return jx, jy


# what select() decided for a foot
STANCE, HELD, CHEAP, LATE, OFF, SELECTED = "stance", "held", "cheap", "late", "off", "selected"


def select(T, cost, P, mask, swing, hold, latch, tile=None):
    """The law.  cost [n_tiles, ny, nx] in swing's dtype.  -> dict(swing, hold, latch: copies advanced; feet: list of dict(state, foot, kind, and for the
    examined feet c0, ok_margin = |c0 - cost_ok| / cost_ok, for the selected ones also J, J2 (second-best; inf with one candidate), margin =
    (J2 - J) / J2, tie = J2 == J, move = the distance from the gait rule's foothold, u = t0 / T, node (ix, iy), clipped: the window met a border))"""
    dt = swing.dtype
    t = dt.type
    assert cost.dtype == dt and hold.dtype == dt
    nz, ny, nx = T["z"].shape
    n = swing.shape[0]
    c = TR.consts(T, dt)
    cell = t(T["cell"])
    tile = np.zeros(n, np.int64) if tile is None else np.asarray(tile, np.int64)
    sw, hd = swing.copy(), hold.copy()
    out = np.zeros(n, np.int32)
    R = int(P["radius"])
    feet = []
    for s in range(n):
        for k in range(4):
            rec = dict(state=s, foot=k)
            feet.append(rec)
            if (int(mask[s]) >> k) & 1:
                rec["kind"] = STANCE
                continue
            if (int(latch[s]) >> k) & 1:
                sw[s, 9 * k + 3], sw[s, 9 * k + 4] = hd[s, 2 * k], hd[s, 2 * k + 1]
                out[s] |= 1 << k
                rec["kind"] = HELD
                continue
            if R == 0:
                rec["kind"] = OFF
                continue
            x, y = sw[s, 9 * k + 3], sw[s, 9 * k + 4]
            jx, jy = (int(a) for a in nearest_node(T, x, y, dt))
            c0 = cost[tile[s], jy, jx]
            rec.update(c0=float(c0), ok_margin=abs(float(c0) - P["cost_ok"]) / P["cost_ok"] if P["cost_ok"] > 0 else np.inf, node0=(jx, jy))
            if c0 <= t(P["cost_ok"]):
                rec["kind"] = CHEAP
                continue
            if sw[s, 9 * k + 8] > t(P["u_max"]) * sw[s, 9 * k + 7]:
                rec["kind"] = LATE
                continue
            ix = np.arange(max(jx - R, 0), min(jx + R, nx - 1) + 1)
            iy = np.arange(max(jy - R, 0), min(jy + R, ny - 1) + 1)
            xc = c["x0"] + ix.astype(dt) * cell
            yc = c["y0"] + iy.astype(dt) * cell
            dx, dy = xc - x, yc - y
            J = cost[tile[s]][np.ix_(iy, ix)] + t(P["w_dist"]) * ((dx * dx)[None, :] + (dy * dy)[:, None])
            assert J.dtype == dt
            b = int(np.argmin(J))                      # the first minimum in scan order: iy outer, ix inner
            by, bx = divmod(b, ix.size)
            Js = np.sort(J.ravel())
            J2 = float(Js[1]) if Js.size > 1 else np.inf
            hd[s, 2 * k], hd[s, 2 * k + 1] = xc[bx], yc[by]
            sw[s, 9 * k + 3], sw[s, 9 * k + 4] = xc[bx], yc[by]
            out[s] |= (1 << k) | (1 << (4 + k))
            rec.update(kind=SELECTED, J=float(Js[0]), J2=J2, margin=(J2 - float(Js[0])) / J2 if J2 > 0 else 0.0, tie=J2 == float(Js[0]),
                       move=float(np.hypot(float(xc[bx]) - float(x), float(yc[by]) - float(y))), u=float(sw[s, 9 * k + 8]) / float(sw[s, 9 * k + 7]),
                       node=(int(ix[bx]), int(iy[by])), clipped=ix.size < 2 * R + 1 or iy.size < 2 * R + 1,
                       window_min=float(cost[tile[s]][np.ix_(iy, ix)].min()))
    return dict(swing=sw, hold=hd, latch=out, feet=feet)


# ---- terrains
RIDGE = 0.02


def ridges(T, period, h=RIDGE):
    """T + ridges of height h along y: column ix of tile t is raised where (ix + 2 t) % 8 == 0 (period 8) or (ix + t) % 4 == 0 (period 4)"""
    z = T["z"].copy()
    nz, ny, nx = z.shape
    for tl in range(nz):
        ix = np.arange(nx)
        z[tl][:, ((ix + 2 * tl) % 8 == 0) if period == 8 else ((ix + tl) % 4 == 0)] += h
    return dict(T, z=z)


def costly_nodes(T):
    """bool [n_tiles, ny, nx]: the node's 3 x 3 neighbourhood holds a height step of more than a millimetre"""
    return cost_map(T, params(margin=1, w_step=1.0, w_slope=0.0))["step"] > 1e-3


COST_GRIDS = ("2x2", "3x2", "5x4", "64x48x4")


def cost_grid(name):
    """the grids of the cost-map tests: terrain_ref.parity_grid's minimal ones, one with interior nodes in both directions and fewer nodes than a
    workgroup's tile, and the walking loop's size with 4 tiles (more than one workgroup each way) carrying ridge4's ridges on the ripple"""
    if name == "5x4":
        return dict(z=np.random.default_rng(synth.SEED + 1590).uniform(-0.05, 0.05, (1, 4, 5)), x0=-0.25, y0=0.5, cell=0.125)
    return ridges(TR.parity_grid(name), 4) if name == "64x48x4" else TR.parity_grid(name)


# ---- a case that takes every branch
BRANCH_SIZES = GR.PARITY_SIZES
KINDS = ("stance", "held", "cheap", "late", "selected", "border", "corner", "nocheap", "tie")


def branch_grid():
    """Three tiles of 24 x 16 nodes, cell 2^-4, origin (-0.5, -0.25).  Tile 0 is never walked on: multiples of 1/8 drawn at random, so that a lost tile
    offset shows.  Tiles 1 and 2 are equal: zero but for
      a ridge of 1/8 along y at column 8 (costly nodes: columns 7, 8, 9), a ridge along y at column 0 (the border) and a raised node at the corner
      (23, 15); columns 14 .. 22 of rows 0 .. 8 alternate 0 and 1/4 (no cheap node in a window inside); and a single raised node (4, 12) of 1/4 whose
      four side neighbours tie exactly when the foot aims at the node itself.
    Every height, the origin, the cell and the weights of branch_params() are dyadic: cost and J are exact in float32 and float64."""
    z = np.zeros((3, 16, 24))
    z[0] = np.random.default_rng(synth.SEED + 1599).integers(0, 5, (16, 24)) / 8.0
    z[1:, :, 8] = 0.125
    z[1:, :, 0] = 0.125
    z[1:, 15, 23] = 0.25
    z[1:, 0:9:2, 14:23] = 0.25
    z[1:, 1:9:2, 14:23:2] = 0.25
    z[1:, 12, 4] = 0.25
    return dict(z=z, x0=-0.5, y0=-0.25, cell=2.0 ** -4)


def branch_params():
    return params(radius=2, margin=1, w_step=1.0, w_slope=0.0, w_dist=4.0, cost_ok=2.0 ** -6, u_max=0.75)


def branch_case(n, rank=0, dtype=np.float64):
    """n states x 4 feet on branch_grid().  Foot (s, k) is of kind KINDS[(s + 2 k + rank) % 9]; from n = 15 on every foot index k meets every kind.
    Off-node aims are node + (fx, fy) cell with fx, fy multiples of 1/16 in [-5/16, 5/16] drawn per foot, except the tie (the node itself).  The other
    swing words are recognisable junk; T = 0.25 and t0 = 0.0625 (u = 0.25), the late kind t0 = 0.21875 (u = 0.875).
    State s walks on tile 1 + s % 2.  -> dict(T, P, mask, swing, hold, latch, tile, kind [n, 4])"""
    T, P = branch_grid(), branch_params()
    rng = np.random.default_rng(synth.SEED + 1600 + rank)
    cell, x0, y0 = T["cell"], T["x0"], T["y0"]
    swing = rng.uniform(-1, 1, (n, 36))
    hold = rng.uniform(-1, 1, (n, 8))
    mask, latch = np.zeros(n, np.int32), np.zeros(n, np.int32)
    kind = np.empty((n, 4), object)
    aim = dict(cheap=(3, 5), late=(8, 6), selected=(8, 5), border=(0, 7), corner=(23, 15), nocheap=(18, 4), tie=(4, 12), held=(8, 9), stance=(8, 3))
    for s in range(n):
        latch[s] |= int(rng.integers(0, 8)) << 4          # bits 4+ on input are not read
        for k in range(4):
            kd = KINDS[(s + 2 * k + rank) % 9]
            kind[s, k] = kd
            ix, iy = aim[kd]
            fx, fy = (0, 0) if kd == "tie" else (int(rng.integers(-5, 6)), int(rng.integers(-5, 6)))
            if kd == "selected":
                iy = int(rng.integers(3, 13))
                fx = fx or 1                              # a foot exactly on the ridge column ties between its two sides
            if kd == "nocheap":
                fx, fy = fx or 1, fy or 1
            if kd == "corner" and fx == fy:
                fy = fy - 1 if fy > -5 else fy + 1        # fx = fy ties between the nodes two cells along x and two cells along y
            swing[s, 9 * k + 3] = x0 + (ix + fx / 16.0) * cell
            swing[s, 9 * k + 4] = y0 + (iy + fy / 16.0) * cell
            swing[s, 9 * k + 7] = 0.25
            swing[s, 9 * k + 8] = 0.21875 if kd == "late" else 0.0625
            if kd == "stance":
                mask[s] |= 1 << k
                if (s + k) % 2 == 0:
                    latch[s] |= 1 << k                    # a stance foot clears a latch
            if kd == "held":
                latch[s] |= 1 << k
    return dict(T=T, P=P, mask=mask, swing=swing.astype(dtype), hold=hold.astype(dtype), latch=latch, tile=(1 + np.arange(n) % 2).astype(np.int32),
                kind=kind)


# ---- the walking loop with selection
WALK_N, WALK_TICKS = TR.WALK_N, TR.WALK_TICKS


def ridge_grids(z0):
    """the two ridge terrains of the walking-loop tests: terrain_ref.walk_grids' flat ground + ridges every 8 / every 4 cells"""
    flat_T = TR.walk_grids(z0)["flat"]
    return {"ridge8": ridges(flat_T, 8), "ridge4": ridges(flat_T, 4)}


def closed_loop(flat, oracle, case, T, P, ticks=WALK_TICKS, k_t=TR.WALK_KT, q0=None):
    """terrain_ref.closed_loop(aware=True) with select() between gait_tick and feet(): per tick gait_tick -> select -> feet(T, q, mask, swing) ->
    oracle.reference -> swing_reference -> oracle.step -> stick_ref.integrate_ground_stick.  P = None: no selection (terrain_ref's loop itself).
    Returns terrain_ref.closed_loop's dict + latches [ticks, N]; selections: list of (tick, the select() record); costly: the share of touchdowns whose
    foot's nearest node is a costly node; aimed_cost: the largest cost of any nearest node a lifted, unlatched foot was examined at; sel_margin: the
    smallest margin of any selection; margin: the smallest cell-edge distance of any FOOT point (cells; a selected foothold is a node, where zs is
    continuous and p1_z exact, so the plans' own samples do not count here); path: the base's xy travel per robot [N, 2]; base_z (min, max over the loop)"""
    prm, G, GP, GPP = synth.default_params(observer_order=0), SR.loop_ref_params(), GR.walk_params(flat), ground_ref.params()
    prm["dt"] = GR.DYADIC_DT
    legs = limit_ref.leg_joints(flat)
    q, v = (case["q"] if q0 is None else q0).copy(), case["v"].copy()
    n = q.shape[0]
    phase, mask, swing = case["phase"].copy(), case["mask"].copy(), case["swing"].copy()
    contact, anchor, stick = np.zeros(n, np.int32), np.zeros((n, 12)), np.zeros(n, np.int32)
    hold, latch = np.zeros((n, 8)), np.zeros(n, np.int32)
    cm = cost_map(T, P if P is not None else params())
    bad = costly_nodes(T)
    rec = dict(masks=[], events=[], contacts=[], latches=[])
    ok, margin, ins, fn_max, touchdowns, selections, aimed, n_costly = True, np.inf, True, 0.0, [], [], 0.0, 0
    qstart, bz = q.copy(), [np.inf, -np.inf]
    for k in range(ticks):
        phase, mask, swing, ev = GR.gait_tick(flat, GP, prm["dt"], q, v, case["cmd"], contact, phase, mask, swing)
        S = select(T, cm["cost"], P if P is not None else params(radius=0), mask, swing, hold, latch, case["tile"])
        for r in S["feet"]:
            if "c0" in r:
                aimed = max(aimed, r["c0"])
            if r["kind"] == SELECTED:
                selections.append((k, r))
        if P is not None:
            swing, hold, latch = S["swing"], S["hold"], S["latch"]
        F = TR.feet(flat, T, q, mask, swing, case["tile"])
        gxy = (F["pf"][:, :, :2] - np.array([T["x0"], T["y0"]])) / T["cell"]
        margin, ins = min(margin, float(np.abs(gxy - np.round(gxy)).min())), ins and F["inside"]
        swing = F["swing"]
        for f in range(4):
            for s in np.nonzero((ev >> (4 + f)) & 1)[0]:
                touchdowns.append((k, int(s), f, float(F["pf"][s, f, 2] - F["surf"][s, f])))
                jx, jy = nearest_node(T, F["pf"][s, f, 0], F["pf"][s, f, 1], np.float64)
                n_costly += bool(bad[case["tile"][s], int(jy), int(jx)])
        ref = oracle.reference(G, q, v, case["plan"], k * prm["dt"])
        vd, _ = SR.swing_reference(flat, q, v, mask, swing, 0.0, ref["vdot_des"], GR.WALK_SWING_PARAMS)
        tick = oracle.step(prm, q, v, ref["w_des"], vd, F["normals"], case["mu"], mask, None, None, None, None)
        ok = ok and bool(np.all(tick["status"] == 0))
        dyn = oracle.dynamics(q, v)
        q, v, g = stick_ref.integrate_ground_stick(GPP, k_t, prm["dt"], dyn, tick["tau"], F["normals"], F["height"], case["mu"], None, q, v, anchor, stick,
                                                   legs)
        anchor, stick, contact = g["anchor"], g["stick"], g["contact"]
        fn_max = max(fn_max, float(g["fn"].max()))
        bz = [min(bz[0], float(q[:, 2].min())), max(bz[1], float(q[:, 2].max()))]
        rec["masks"].append(mask.copy()); rec["events"].append(ev.copy()); rec["contacts"].append(contact.copy()); rec["latches"].append(latch.copy())
    gaps = np.array([t[3] for t in touchdowns])
    out = dict(q=q, v=v, status_ok=ok, touchdowns=touchdowns, gap_max=float(np.abs(gaps).max()), fn_max=fn_max, margin=margin, inside=ins,
               selections=selections, costly=n_costly / max(1, len(touchdowns)), aimed_cost=aimed,
               sel_margin=min([r["margin"] for _, r in selections], default=np.inf), path=(q - qstart)[:, :2], base_z=tuple(bz))
    out.update({key: np.array(val) for key, val in rec.items()})
    return out


def cpu_walk(flat, oracle, terrain="ridge8", select_on=True):
    """(case with case["T"], case["P"]; closed_loop(case)) of WALK_N robots on a ridge terrain (or terrain_ref.walk_grids' "flat" / "tiles"), computed once
    per process and shared by the tests that need it: read only"""
    def make():
        c = TR.walk_case(flat, oracle)
        c["T"] = dict(TR.walk_grids(c["z0"]), **ridge_grids(c["z0"]))[terrain]
        c["P"] = params() if select_on else None
        return c
    return walk_ref.cached(("foothold", id(flat), terrain, bool(select_on)), make, lambda case: closed_loop(flat, oracle, case, case["T"], case["P"]))


# amplification of a 1e-12 relative perturbation of q0 over the selecting walking loop on the period-8 ridges, measured by
# tests/test_foothold_oracle.py (1.52), rounded up: the device loop's gate in tests/test_gpu_foothold.py is max(1e-6, 10 A 1e-9), the rule of
# tests/test_gpu_ground.py
WALK_AMPLIFICATION = 2.0
