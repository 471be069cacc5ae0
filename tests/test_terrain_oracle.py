"""The numpy restatement of the terrain heightfield (tests/terrain_ref.py) against what the law must give on grids whose answer is known, and the
walking loop that says why the feature exists.  No GPU.

The walking loop (terrain_ref.closed_loop: 4 robots, 512 ticks of 2^-10 s, the stiction plant with k_t 2e4, sensed = the plant's word; 4 tiles of
64 x 48 nodes, cell 2^-6, origin (-0.5, -0.375), tile t: z0 + 0.05 x + 0.006 sin(2 pi (x / 0.125 + t / 4)) cos(2 pi y / 0.25)).  Measured, gap =
p_f,z - zs(p_f,xy) of a foot at the tick of its touchdown event, 32 events per loop:
  flat ground, aware   -0.04 ... +0.61 mm, largest f_n 290 N
  tiles, aware         -0.13 ... +0.80 mm, largest f_n 524 N     (1.3 x flat)
  tiles, blind         -1.86 ... +14.91 mm, largest f_n 779 N    (18.7 x aware)
every QP status 0 in all three.  Smallest distance of any sample's gx, gy from an integer in the aware loop: 2.0e-5 cells (x0, y0 were not moved); every
sampled point inside the grid.  Amplification of a 1e-12 relative perturbation of q0 through the aware loop A = 2.7 (mask, event and contact words
equal between the two runs); terrain_ref.WALK_AMPLIFICATION = 3."""
import numpy as np
import pytest

from tests import terrain_ref as R

# dyadic plane and grid: every node, every product and every sum of the law is exact in float64
PLANE = dict(c=0.375, a=0.25, b=-0.125)
GRID = dict(nx=9, ny=5, x0=-0.5, y0=-0.25, cell=0.125)


def _plane(x, y, t=0):
    return PLANE["c"] + t / 8.0 + PLANE["a"] * x + PLANE["b"] * y


def _grid(n_tiles=1, **kw):
    g = dict(GRID, **kw)
    return R.grid_plane(g["nx"], g["ny"], g["x0"], g["y0"], g["cell"], PLANE["c"], PLANE["a"], PLANE["b"], n_tiles)


def _normal():
    n = np.array([-PLANE["a"], -PLANE["b"], 1.0])
    return n / np.linalg.norm(n)


def _check_plane(T, x, y, tile=None, t_of=0):
    s = R.sample(T, x, y, tile)
    nz, ny, nx = T["z"].shape
    xc = np.clip(x, T["x0"], T["x0"] + (nx - 1) * T["cell"])
    yc = np.clip(y, T["y0"], T["y0"] + (ny - 1) * T["cell"])
    c = PLANE["c"] + np.asarray(t_of) / 8.0
    assert np.abs(s["z"] - _plane(xc, yc, np.asarray(t_of))).max() <= 1e-12
    assert np.abs(s["n"] - _normal()[None, :]).max() <= 1e-12
    assert np.abs(s["d"] - c * _normal()[2]).max() <= 1e-12
    return s


def test_plane_identity_inside_the_grid():
    T = _grid()
    rng = np.random.default_rng(11)
    xm, ym = GRID["x0"] + (GRID["nx"] - 1) * GRID["cell"], GRID["y0"] + (GRID["ny"] - 1) * GRID["cell"]
    x, y = rng.uniform(GRID["x0"], xm, 400), rng.uniform(GRID["y0"], ym, 400)
    s = _check_plane(T, x, y)
    assert set(s["ix"]) == set(range(GRID["nx"] - 1)) and set(s["iy"]) == set(range(GRID["ny"] - 1))      # every cell, the last ones included
    # at grid nodes -- the last row and column included, where u = 1 or w = 1 -- zs is the node bit for bit
    I, J = np.meshgrid(np.arange(GRID["nx"]), np.arange(GRID["ny"]))
    xn, yn = GRID["x0"] + GRID["cell"] * I.ravel(), GRID["y0"] + GRID["cell"] * J.ravel()
    sn = R.sample(T, xn, yn)
    assert np.array_equal(sn["z"], T["z"][0].ravel())
    assert np.array_equal(sn["ix"], np.minimum(I.ravel(), GRID["nx"] - 2)) and np.array_equal(sn["iy"], np.minimum(J.ravel(), GRID["ny"] - 2))


def test_points_off_the_grid_see_the_plane_at_the_clamped_point():
    T = _grid()
    xm, ym = GRID["x0"] + (GRID["nx"] - 1) * GRID["cell"], GRID["y0"] + (GRID["ny"] - 1) * GRID["cell"]
    xi, yi = GRID["x0"] + 0.3, GRID["y0"] + 0.2
    pts = [(GRID["x0"] - 1.0, yi), (xm + 1.0, yi), (xi, GRID["y0"] - 2.0), (xi, ym + 0.5),                                   # each edge
           (GRID["x0"] - 1.0, GRID["y0"] - 1.0), (xm + 1.0, GRID["y0"] - 1.0), (GRID["x0"] - 1.0, ym + 1.0), (xm + 1.0, ym + 1.0)]   # each corner
    x, y = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    s = _check_plane(T, x, y)
    assert list(s["ix"][[0, 1]]) == [0, GRID["nx"] - 2] and list(s["iy"][[2, 3]]) == [0, GRID["ny"] - 2]
    # on a curved grid: the height beyond an edge is the height AT the edge, and n, d are those of the edge point
    C = R.parity_grid("3x2")
    far = R.sample(C, np.array([5.0, -5.0]), np.array([0.6, 0.7]))
    edge = R.sample(C, np.array([C["x0"] + 2 * C["cell"], C["x0"]]), np.array([0.6, 0.7]))
    for key in ("z", "n", "d"):
        assert np.array_equal(far[key], edge[key]), key


@pytest.mark.parametrize("name", R.PARITY_GRIDS)
def test_branch_case_takes_every_branch(name):
    """interior, each clamp side, the last cell, nodes, every tile -- on the minimal grid nx = ny = 2 too -- with the margins the device tests assert"""
    T = R.parity_grid(name)
    nz, ny, nx = T["z"].shape
    c = R.branch_case(T, 33, rank=33)
    s = R.sample(T, c["x"], c["y"], c["tile"])
    s32 = R.sample(T, c["x"].astype(np.float32), c["y"].astype(np.float32), c["tile"])
    xm, ym = T["x0"] + (nx - 1) * T["cell"], T["y0"] + (ny - 1) * T["cell"]
    assert (c["x"] < T["x0"]).any() and (c["x"] > xm).any() and (c["y"] < T["y0"]).any() and (c["y"] > ym).any()
    assert ((c["x"] < T["x0"]) & (c["y"] > ym)).any() and ((c["x"] > xm) & (c["y"] < T["y0"])).any()
    assert ((s["ix"] == nx - 2) & (s["iy"] == ny - 2) & ~c["node"]).any() and c["node"].sum() >= 4
    assert set(c["tile"]) == set(range(nz))
    free = ~c["node"] & (c["x"] > T["x0"]) & (c["x"] < xm) & (c["y"] > T["y0"]) & (c["y"] < ym)
    assert free.sum() >= 10
    pick = lambda r: {key: r[key][free] for key in ("gx", "gy", "cx", "cy")}
    assert R.edge_margin(pick(s)) >= R.MARGIN64 and R.edge_margin(pick(s32)) >= R.MARGIN32
    assert np.array_equal(s["ix"], s32["ix"]) and np.array_equal(s["iy"], s32["iy"])          # the same cells in both scalar types
    # nodes: u, w are exactly 0 or 1; with u = w = 0 zs is the node's own bits in both scalar types, on the last row and column to two roundings
    for r, zt, eps in ((s, T["z"], 2.0 ** -52), (s32, T["z"].astype(np.float32), 2.0 ** -23)):
        assert np.all(np.isin(r["u"][c["node"]], (0, 1)) & np.isin(r["w"][c["node"]], (0, 1)))
        I = np.rint((c["x"] - T["x0"]) / T["cell"]).astype(int); J = np.rint((c["y"] - T["y0"]) / T["cell"]).astype(int)
        assert c["node0"].any() and np.array_equal(r["z"][c["node0"]], zt[c["tile"][c["node0"]], J[c["node0"]], I[c["node0"]]])
        assert np.abs(r["z"][c["node"]] - zt[c["tile"][c["node"]], J[c["node"]], I[c["node"]]]).max() <= 4 * eps * np.abs(zt).max()
    # float32 against float64: what single precision costs stays inside the device tests' fp32 gate
    for key in ("z", "n", "d"):
        assert np.abs(s32[key] - s[key]).max() <= 5e-4 * np.abs(s[key]).max(), key


def test_minimal_grid_and_tiles_on_a_plane():
    T = _grid(n_tiles=3, nx=2, ny=2, cell=0.5)
    rng = np.random.default_rng(12)
    x, y = rng.uniform(-1.0, 0.5, 60), rng.uniform(-0.75, 0.75, 60)
    tile = np.arange(60) % 3
    s = _check_plane(T, x, y, tile, t_of=tile)
    assert np.all(s["ix"] == 0) and np.all(s["iy"] == 0)


def test_feet_writes_planes_and_only_p1z_of_lifted_feet(flat_model):
    from tests import gait_ref as GR, swing_ref as SR
    from wbc_quadruped_dob_amd import synth
    n = 33
    c = GR.branch_case(flat_model, float(np.sum(flat_model["mass"])), n, rank=n)
    T = R.parity_grid("64x48x4")
    mask = SR.all_masks(n)
    tile = (np.arange(n) % 4).astype(np.int32)
    F = R.feet(flat_model, T, c["q"], mask, c["swing"], tile)
    P = R.feet(flat_model, T, c["q"], None, None, tile)
    for key in ("normals", "height", "surf"):
        assert np.array_equal(F[key], P[key]), key
    assert P["swing"] is None
    changed = F["swing"] != c["swing"]
    for k in range(4):
        air = ((mask >> k) & 1) == 0
        cols = np.zeros(36, bool); cols[9 * k + 5] = True
        assert changed[np.ix_(air, cols)].all() and not changed[np.ix_(air, ~cols)][:, 9 * k:9 * k + 8].any()
        assert not changed[~air, 9 * k:9 * k + 9].any()
    assert np.abs(np.linalg.norm(F["normals"].reshape(n, 4, 3), axis=2) - 1).max() < 1e-14
    # d is the plane through the surface point under the foot
    again = R.feet(flat_model, T, c["q"], mask, F["swing"], tile)
    assert np.array_equal(again["swing"], F["swing"])          # idempotent


def test_walking_loop_lands_on_the_map(flat_model, oracle):
    """The docstring's figures.  First the conditions the reference alone must meet (cell-edge margin of every sample, every foot inside the grid);
    then: the aware loop solves every QP; its largest touchdown gap is at most 1.5 x flat ground's; the blind loop's is at least 5 x the aware one's."""
    case, aware = R.cpu_walk(flat_model, oracle, "tiles", True)
    assert aware["margin"] >= R.MARGIN64, aware["margin"]
    assert aware["inside"]
    _, flat = R.cpu_walk(flat_model, oracle, "flat", True)
    _, blind = R.cpu_walk(flat_model, oracle, "tiles", False)
    for name, w in (("flat aware", flat), ("tiles aware", aware), ("tiles blind", blind)):
        print("%s: gap %.3f ... %.3f mm, largest |gap| %.3f mm, largest f_n %.0f N, %d touchdowns, status_ok %s, margin %.3g cells"
              % (name, 1e3 * w["gap_range"][0], 1e3 * w["gap_range"][1], 1e3 * w["gap_max"], w["fn_max"], len(w["touchdowns"]), w["status_ok"], w["margin"]))
    assert aware["status_ok"]
    assert len(aware["touchdowns"]) == 32 and len(flat["touchdowns"]) == 32
    assert set(case["tile"]) == {0, 1, 2, 3}
    assert aware["gap_max"] <= 1.5 * flat["gap_max"]
    assert blind["gap_max"] >= 5 * aware["gap_max"]


def test_walking_loop_sensitivity(flat_model, oracle):
    """A = |delta end| / |delta start| for q0 perturbed by 1e-12 relative: tests/test_gpu_terrain.py derives its closed-loop gate from it"""
    case, cpu = R.cpu_walk(flat_model, oracle, "tiles", True)
    q0 = case["q"] * (1 + 1e-12 * np.random.default_rng(1).uniform(-1, 1, case["q"].shape))
    p = R.closed_loop(flat_model, oracle, case, case["T"], True, q0=q0)
    d0 = np.abs(q0 - case["q"]).max()
    d1 = max(np.abs(p["q"] - cpu["q"]).max(), np.abs(p["v"] - cpu["v"]).max())
    A = d1 / d0
    print("A = %.3g (start %.3g, end %.3g)" % (A, d0, d1))
    for k in ("masks", "events", "contacts"):
        assert np.array_equal(p[k], cpu[k]), k
    assert A <= R.WALK_AMPLIFICATION
