"""The numpy restatement of the foothold selection (tests/foothold_ref.py) against per-node and per-candidate Python loops, the branch case the device
tests run, and the walking loops that say why the feature exists and how its defaults were fixed.  No GPU.

The walking loop (foothold_ref.closed_loop: terrain_ref's loop -- 4 robots, 512 ticks of 2^-10 s, the stiction plant, sensed = the plant's word -- with
the selection between the gait rule and the terrain rule; terrain_ref.walk_grids' flat ground, 4 tiles of 64 x 48 nodes, cell 2^-6, + 2 cm ridges along
y at the columns (ix + 2 t) % 8 == 0 or (ix + t) % 4 == 0 of tile t).  A touchdown is costly when the node nearest to the foot at the tick of its
touchdown event has a height step in its 3 x 3 neighbourhood.  Measured with the defaults (32 touchdowns per loop, every QP status 0 in all four):
  ridges every 8, off   41 % costly; forward 4.79 .. 4.92 cm, sideways within 1.7 mm, base height 0.398 .. 0.405 m
  ridges every 8, on     0 % costly; forward 4.72 .. 4.78 cm, sideways within 2.0 mm, base height 0.398 .. 0.406 m; 19 selections, the latest at
                        u = 0.484, the largest move 2.97 cm, the smallest margin (J2 - J) / J2 = 1.67e-4, every |c0 - cost_ok| / cost_ok >= 1.29
  ridges every 4, off   84 % costly; robot 1 walks 1.66 cm forward and 2.75 cm sideways, robot 3 8.23 cm forward, base height down to 0.386 m
  ridges every 4, on     0 % costly; forward 4.53 .. 4.94 cm, sideways within 2.2 mm, base height 0.398 .. 0.407 m; 38 selections, the latest at
                        u = 0.453, the largest move 2.97 cm, the smallest margin 4.03e-3
How w_slope and cost_ok were fixed (include/wbc_hip.h): the largest cost of a node a foot is aimed at on "flat" is 0 and on "tiles" 5.024e-3 with
w_slope = 0, 5.832e-3 with 2^-7, 6.639e-3 with 2^-6, 8.255e-3 with 2^-5; times 1.5: 7.54e-3, 8.75e-3, 9.96e-3, 1.24e-2.  The cheapest ridge-adjacent node
costs 0.02 (the ridge's own nodes: their central difference is 0), so cost_ok must lie below 0.01: 2^-5 fails, 2^-6 leaves 0.4 %, 2^-7 leaves 12.5 % and
is the default, with cost_ok = 8.75e-3.
Amplification of a 1e-12 relative perturbation of q0 through the selecting loop on the ridges every 8: A = 1.52 (mask, event, contact
and latch words equal between the two runs); foothold_ref.WALK_AMPLIFICATION = 2."""
import numpy as np
import pytest

from tests import foothold_ref as R, terrain_ref as TR


# ---- cost map
def _cost_loop(T, P):
    """per node, in Python floats"""
    z = T["z"]
    nz, ny, nx = z.shape
    inv = 1.0 / T["cell"]
    m = P["margin"]
    clip = lambda i, n: min(max(i, 0), n - 1)
    step, cost = np.zeros_like(z), np.zeros_like(z)
    for t in range(nz):
        for iy in range(ny):
            for ix in range(nx):
                s = 0.0
                for dy in range(-m, m + 1):
                    for dx in range(-m, m + 1):
                        s = max(s, abs(z[t, clip(iy + dy, ny), clip(ix + dx, nx)] - z[t, iy, ix]))
                sx = (z[t, iy, ix + 1] - z[t, iy, ix - 1]) * inv / 2 if 0 < ix < nx - 1 else \
                    ((z[t, iy, 1] - z[t, iy, 0]) if ix == 0 else (z[t, iy, nx - 1] - z[t, iy, nx - 2])) * inv
                sy = (z[t, iy + 1, ix] - z[t, iy - 1, ix]) * inv / 2 if 0 < iy < ny - 1 else \
                    ((z[t, 1, ix] - z[t, 0, ix]) if iy == 0 else (z[t, ny - 1, ix] - z[t, ny - 2, ix])) * inv
                step[t, iy, ix] = s
                cost[t, iy, ix] = P["w_step"] * s + P["w_slope"] * (sx * sx + sy * sy)
    return step, cost


@pytest.mark.parametrize("name", R.COST_GRIDS)
def test_cost_map_against_a_per_node_loop(name):
    T = R.cost_grid(name)
    for margin in ((1,) if name == "64x48x4" else (0, 1, 2)):
        P = R.params(margin=margin, w_slope=0.375)
        step, cost = _cost_loop(T, P)
        cm = R.cost_map(T, P)
        assert np.array_equal(cm["step"], step), margin           # subtraction, abs and max only: bit for bit
        assert np.array_equal(cm["cost"], cost), margin           # and here the products are the same roundings too
        assert np.array_equal(R.cost_map(T, dict(P, w_slope=0.0))["cost"], step)
        assert (step > 0).any() or margin == 0
        if margin == 0:
            assert not step.any()
    c32 = R.cost_map(T, R.params(w_slope=0.375), np.float32)["cost"]
    assert c32.dtype == np.float32 and np.abs(c32 - R.cost_map(T, R.params(w_slope=0.375))["cost"]).max() <= 5e-4 * cost.max()


def test_costly_nodes_of_the_ridge_terrains():
    flat_T = TR.walk_grids(0.0)["flat"]
    for period, share in ((8, 3 / 8), (4, 3 / 4)):
        bad = R.costly_nodes(R.ridges(flat_T, period))
        assert abs(bad.mean() - share) < 0.01          # a ridge column and its two neighbours (a grid border cuts one of them)
        cm = R.cost_map(R.ridges(flat_T, period), R.params())
        assert cm["cost"][bad].min() == R.RIDGE and not cm["cost"][~bad].any()
        assert R.DEFAULTS["cost_ok"] < 0.5 * cm["cost"][bad].min()


# ---- selection
def _select_loop(T, cost, P, mask, swing, hold, latch, tile):
    """per foot and per candidate, in the arithmetic of swing's dtype"""
    t = swing.dtype.type
    nz, ny, nx = T["z"].shape
    x0, y0, cell, inv = t(T["x0"]), t(T["y0"]), t(T["cell"]), t(1.0 / T["cell"])
    sw, hd, out = swing.copy(), hold.copy(), np.zeros_like(latch)
    for s in range(swing.shape[0]):
        for k in range(4):
            if (mask[s] >> k) & 1:
                continue
            if (latch[s] >> k) & 1:
                sw[s, 9 * k + 3:9 * k + 5] = hd[s, 2 * k:2 * k + 2]
                out[s] |= 1 << k
                continue
            x, y = sw[s, 9 * k + 3], sw[s, 9 * k + 4]
            jx = min(max(int(np.floor((x - x0) * inv + t(0.5))), 0), nx - 1)
            jy = min(max(int(np.floor((y - y0) * inv + t(0.5))), 0), ny - 1)
            if P["radius"] == 0 or cost[tile[s], jy, jx] <= t(P["cost_ok"]) or sw[s, 9 * k + 8] > t(P["u_max"]) * sw[s, 9 * k + 7]:
                continue
            best = None
            for iy in range(jy - P["radius"], jy + P["radius"] + 1):
                for ix in range(jx - P["radius"], jx + P["radius"] + 1):
                    if not (0 <= ix < nx and 0 <= iy < ny):
                        continue
                    xc, yc = x0 + t(ix) * cell, y0 + t(iy) * cell
                    J = cost[tile[s], iy, ix] + t(P["w_dist"]) * ((xc - x) * (xc - x) + (yc - y) * (yc - y))
                    if best is None or J < best[0]:
                        best = (J, xc, yc)
            hd[s, 2 * k], hd[s, 2 * k + 1] = best[1], best[2]
            sw[s, 9 * k + 3], sw[s, 9 * k + 4] = best[1], best[2]
            out[s] |= (1 << k) | (1 << (4 + k))
    return sw, hd, out


def _random_case(n, dtype, seed):
    """feet aimed anywhere on (and a little beyond) ridge4 on the rippled 64 x 48 x 4 grid, every mask, random latches and swing times"""
    from tests import swing_ref as SR
    T = R.cost_grid("64x48x4")
    rng = np.random.default_rng(seed)
    swing = rng.uniform(-1, 1, (n, 36))
    for k in range(4):
        swing[:, 9 * k + 3] = rng.uniform(T["x0"] - 0.03, T["x0"] + 63 * T["cell"] + 0.03, n)
        swing[:, 9 * k + 4] = rng.uniform(T["y0"] - 0.03, T["y0"] + 47 * T["cell"] + 0.03, n)
        swing[:, 9 * k + 7] = 0.25
        swing[:, 9 * k + 8] = rng.uniform(0, 0.25, n)
    return dict(T=T, mask=SR.all_masks(n), swing=swing.astype(dtype), hold=rng.uniform(-1, 1, (n, 8)).astype(dtype),
                latch=rng.integers(0, 256, n).astype(np.int32), tile=(np.arange(n) % 4).astype(np.int32))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_selection_against_a_brute_force_loop(dtype):
    cases = [(R.branch_case(33, rank=33, dtype=dtype), R.branch_params())]
    cases += [(_random_case(64, dtype, 7 + r), P) for r, P in enumerate((R.params(), R.params(radius=4, margin=2, w_slope=0.1), R.params(radius=0),
                                                                          R.params(radius=1, u_max=0.25)))]
    for c, P in cases:
        cost = R.cost_map(c["T"], P, dtype)["cost"]
        S = R.select(c["T"], cost, P, c["mask"], c["swing"], c["hold"], c["latch"], c["tile"])
        sw, hd, la = _select_loop(c["T"], cost, P, c["mask"], c["swing"], c["hold"], c["latch"], c["tile"])
        assert np.array_equal(S["swing"], sw) and np.array_equal(S["hold"], hd) and np.array_equal(S["latch"], la)
        kinds = {r["kind"] for r in S["feet"]}
        assert kinds >= ({R.STANCE, R.HELD, R.OFF} if P["radius"] == 0 else {R.STANCE, R.HELD, R.CHEAP, R.LATE, R.SELECTED}), kinds
        if P["radius"] == 0:
            assert not (S["latch"] >> 4).any() and np.array_equal(S["hold"], c["hold"])


def _branch_records(n, dtype):
    c = R.branch_case(n, rank=n, dtype=dtype)
    cost = R.cost_map(c["T"], c["P"], dtype)["cost"]
    return c, cost, R.select(c["T"], cost, c["P"], c["mask"], c["swing"], c["hold"], c["latch"], c["tile"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("n", R.BRANCH_SIZES)
def test_branch_case_takes_every_branch_with_margins(n, dtype):
    """every kind on every foot from n = 15 on; every decision clear by foothold_ref.MARGIN except the tie, which is exact and goes to the first
    candidate in scan order; no foot left out"""
    c, cost, S = _branch_records(n, dtype)
    nz, ny, nx = c["T"]["z"].shape
    assert len(S["feet"]) == 4 * n
    expect = dict(stance=R.STANCE, held=R.HELD, cheap=R.CHEAP, late=R.LATE)
    for r in S["feet"]:
        s, k = r["state"], r["foot"]
        kd = c["kind"][s, k]
        assert r["kind"] == expect.get(kd, R.SELECTED), (kd, r)
        if "ok_margin" in r:
            assert r["ok_margin"] >= R.MARGIN, r
        if r["kind"] != R.SELECTED:
            assert not (S["latch"][s] >> (4 + k)) & 1 and ((S["latch"][s] >> k) & 1) == (kd == "held")
            cols = slice(9 * k, 9 * k + 9)
            if kd == "held":
                assert np.array_equal(S["swing"][s, 9 * k + 3:9 * k + 5], c["hold"][s, 2 * k:2 * k + 2])
            else:
                assert np.array_equal(S["swing"][s, cols], c["swing"][s, cols])
            continue
        assert (S["latch"][s] >> k) & 1 and (S["latch"][s] >> (4 + k)) & 1
        ix, iy = r["node"]
        assert S["hold"][s, 2 * k] == c["T"]["x0"] + ix * c["T"]["cell"] and S["hold"][s, 2 * k + 1] == c["T"]["y0"] + iy * c["T"]["cell"]   # exact: dyadic
        if kd == "tie":
            assert r["tie"] and r["node"] == (4, 10), r          # of (4, 10), (2, 12), (6, 12), (4, 14) the scan meets (4, 10) first
        else:
            assert not r["tie"] and r["margin"] >= R.MARGIN, r
        if kd == "border":
            assert r["clipped"] and r["node0"][0] == 0
        if kd == "corner":
            assert r["clipped"] and r["node0"] == (nx - 1, ny - 1)
        if kd == "nocheap":
            assert r["window_min"] > c["P"]["cost_ok"] and not r["clipped"]
        if kd in ("selected", "border", "corner", "tie"):
            assert cost[c["tile"][s], iy, ix] <= c["P"]["cost_ok"]
    if n >= 15:
        for k in range(4):
            assert {c["kind"][s, k] for s in range(n)} == set(R.KINDS), k
        stance = [(s, k) for s in range(n) for k in range(4) if c["kind"][s, k] == "stance"]
        assert any((c["latch"][s] >> k) & 1 for s, k in stance) and not any((S["latch"][s] >> k) & 1 for s, k in stance)   # stance clears a latch
    # words no rule names are untouched
    other = np.ones(36, bool)
    other[[9 * k + j for k in range(4) for j in (3, 4)]] = False
    assert np.array_equal(S["swing"][:, other], c["swing"][:, other])


def test_both_scalar_types_decide_alike():
    for n in R.BRANCH_SIZES:
        a, b = _branch_records(n, np.float64)[2], _branch_records(n, np.float32)[2]
        assert np.array_equal(a["latch"], b["latch"])
        picked = np.repeat(((a["latch"][:, None] >> (4 + np.arange(4))) & 1).astype(bool), 2, axis=1)      # rows 2k, 2k+1 of the feet selected
        assert np.array_equal(a["hold"][picked], b["hold"].astype(np.float64)[picked])                      # nodes of a dyadic grid: exact in both


# ---- the walking loops
FIGURES = {   # terrain: (latest u of a selection, largest move [m], smallest margin) -- bounds just beyond the measured figures of the docstring
    "ridge8": (0.49, 0.030, 1.6e-4),
    "ridge4": (0.46, 0.030, 4.0e-3),
}


@pytest.mark.parametrize("terrain", sorted(FIGURES))
def test_ridge_loops(flat_model, oracle, terrain):
    """the docstring's figures"""
    case, on = R.cpu_walk(flat_model, oracle, terrain, True)
    _, off = R.cpu_walk(flat_model, oracle, terrain, False)
    sel = [r for _, r in on["selections"]]
    u_last, move, margin = max(r["u"] for r in sel), max(r["move"] for r in sel), on["sel_margin"]
    for name, w in (("off", off), ("on", on)):
        print("%s %s: costly %.3f of %d, status_ok %s, forward %.2f .. %.2f cm, sideways within %.2f mm, base z %.4f .. %.4f, %d selections"
              % (terrain, name, w["costly"], len(w["touchdowns"]), w["status_ok"], 100 * w["path"][:, 0].min(), 100 * w["path"][:, 0].max(),
                 1e3 * np.abs(w["path"][:, 1]).max(), w["base_z"][0], w["base_z"][1], len(w["selections"])))
    print("latest u %.4f, largest move %.4f m, smallest margin %.3g, smallest ok_margin %.3g, foot-point edge margin %.3g cells"
          % (u_last, move, margin, min(r["ok_margin"] for r in sel), on["margin"]))
    assert set(case["tile"]) == {0, 1, 2, 3}
    assert on["status_ok"] and off["status_ok"]
    assert len(on["touchdowns"]) == 32 and len(off["touchdowns"]) == 32
    assert off["costly"] >= 0.3 and not off["selections"]
    assert on["costly"] == 0.0
    assert u_last <= FIGURES[terrain][0] and move <= FIGURES[terrain][1] and margin >= FIGURES[terrain][2]
    assert on["inside"] and on["margin"] >= TR.MARGIN64
    # a latched point is held until the foot is down: between a selection and the foot's next touchdown the plan's p1 does not move
    assert all(abs(p) < 0.003 for p in on["path"][:, 1]) and np.all(on["path"][:, 0] > 0.045)
    # every selected node is cheap, and the foot lands on it
    assert all(r["J"] - 4.0 * r["move"] ** 2 <= case["P"]["cost_ok"] for r in sel)


def test_ridge_loop_sensitivity(flat_model, oracle):
    """A = |delta end| / |delta start| for q0 perturbed by 1e-12 relative: tests/test_gpu_foothold.py derives its closed-loop gate from it"""
    case, cpu = R.cpu_walk(flat_model, oracle, "ridge8", True)
    q0 = case["q"] * (1 + 1e-12 * np.random.default_rng(1).uniform(-1, 1, case["q"].shape))
    p = R.closed_loop(flat_model, oracle, case, case["T"], case["P"], q0=q0)
    d0 = np.abs(q0 - case["q"]).max()
    d1 = max(np.abs(p["q"] - cpu["q"]).max(), np.abs(p["v"] - cpu["v"]).max())
    A = d1 / d0
    print("A = %.3g (start %.3g, end %.3g)" % (A, d0, d1))
    for k in ("masks", "events", "contacts", "latches"):
        assert np.array_equal(p[k], cpu[k]), k
    assert A <= R.WALK_AMPLIFICATION


@pytest.mark.parametrize("terrain", ["flat", "tiles"])
def test_defaults_never_select_on_flat_ground_and_the_tiles(flat_model, oracle, terrain):
    """the rule that fixed cost_ok: no node a foot is aimed at exceeds it, so the loop is terrain_ref's own, bit for bit"""
    case, w = R.cpu_walk(flat_model, oracle, terrain, True)
    _, ref = TR.cpu_walk(flat_model, oracle, terrain, True)
    print("%s: largest cost aimed at %.6g, cost_ok %.6g" % (terrain, w["aimed_cost"], case["P"]["cost_ok"]))
    assert not w["selections"] and not w["latches"].any()
    assert 1.5 * w["aimed_cost"] <= case["P"]["cost_ok"]
    for k in ("q", "v", "masks", "events", "contacts"):
        assert np.array_equal(w[k], ref[k]), k
