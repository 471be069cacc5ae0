"""GPU: the QP of the cold fp64 observer-off one-launch tick with fewer instructions around the same arithmetic (csrc/qp_struct16.hip.hpp, DIET:
the loop tested at its bottom on `ip` alone, table addresses the compiler cannot fold, the tail's addresses formed early, the drop path's scratch read
by every row, write-through last stores).  None of it may change a bit: f, status, iters -- and tau when M, h, Jc are not asked for -- are compared
bit for bit with the two-launch tick of the same solver (fused_max = 0), whose QP kernel keeps the plain form, and everything is held against the CPU
oracle at the gates of tests/util.py.  It passes on the parent build too.

What the wave-uniform branches and the row selects do depends on which rows share a wavefront: one wavefront of four rows (N = 4), a full workgroup (16),
a ragged one whose last state is the only live row of its wavefront (17), four workgroups (64) -- with and without M, h, Jc.

Input sets (64 states each, every size takes the first rows):
  standing  the benchmark's family (4-contact stance);
  hard      tests/test_gpu_trip_skip.py's: low friction, lateral commands, tight force box, tilted normals; first half in 4-contact stance;
  trot      the same demands under the trot masks only: 2- and 3-foot stances, so that the drops leave 0, 1 and 2 rows on a foot;
  limit     `hard` with max_iter = 9: rows stopped in mid-iteration (status 1);
  infeasible `hard` with one state (16: alone in its wavefront at N = 17) that admits no normal force (status 2), reached over dual-only steps.
That these situations ARE in the inputs is asserted first, on the CPU, from the trace of tools/structured_gi.py (the numpy restatement of the kernel's
iteration: one letter per trip -- A full step, P partial step + drop, D dual-only step + drop -- and per drop the rows left on its foot): partial and
dual-only trips, drops leaving 0, 1 and 2 rows, and two rows of one wavefront dropping in the same trip (a row's k-th trip is its wavefront's k-th)."""
import importlib.util
import os

import numpy as np
import pytest

from tests.test_gpu_parity import _run_step, _solver
from tests.util import elementwise_excess, relerr
from wbc_quadruped_dob_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIZES = (4, 16, 17, 64)
NMAX = max(SIZES)
HARD = dict(fn_max=90.0, fn_min=5.0)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _batch(total_mass, which):
    if which == "standing":
        return synth.make_batch(2, NMAX, total_mass, rank=78), {}
    n = NMAX
    trot = which == "trot"
    rng = np.random.default_rng(123 if trot else 99)
    B = synth.make_batch(4, n, total_mass, rank=47 if trot else 31)
    B["mu"] = rng.choice([0.15, 0.25, 0.4], size=(n, 4))
    B["w_des"][:, 0:2] += rng.uniform(-180, 180, (n, 2))
    B["w_des"][:, 3:6] += rng.uniform(-40, 40, (n, 3))
    if not trot:
        B["mask"][: n // 2] = 0b1111
    if which == "infeasible":
        B["mu"][16] = -0.3
    return B, dict(HARD)


def _traces(oracle, P, B):
    """per state: the trips of its iteration and its drops (tools/structured_gi.py)"""
    spec = importlib.util.spec_from_file_location("structured_gi", os.path.join(ROOT, "tools", "structured_gi.py"))
    sg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sg)
    dyn = oracle.dynamics(B["q"], B["v"])
    tr, dr = [], []
    for i in range(B["q"].shape[0]):
        d = dyn["pf"][i].reshape(4, 3) - B["q"][i, :3]
        s = sg.StructuredGI(np.asarray(P["S"], float), P["alpha"], int(B["mask"][i]), d, B["normals"][i].reshape(4, 3), B["mu"][i] * P["mu_scale"],
                            P["fn_min"], P["fn_max"], B["w_des"][i], tol=P["qp_tol"], max_iter=P["max_iter"])
        s.solve()
        tr.append("".join(s.trace))
        dr.append(list(s.drops))
    return tr, dr


def situations(tr, dr, n):
    """what the first n states' iterations hold: the letters seen, the numbers of rows a drop left on its foot, and whether two rows of one wavefront
    (four consecutive states) drop in the same trip"""
    letters = set("".join(tr[:n]))
    left = {q for d in dr[:n] for _, q in d}
    pair = False
    for w in range(0, n, 4):
        seen = {}
        for i in range(w, min(w + 4, n)):
            for t in {t for t, _ in dr[i]}:
                seen[t] = seen.get(t, 0) + 1
        pair = pair or any(c >= 2 for c in seen.values())
    return letters, left, pair


_cache = {}


def _case(gpu_model, oracle, which, **kw):
    """per input set and parameters, once for the module: the two solvers, the batch, the oracle's answer, the traces and the drops"""
    key = (which,) + tuple(sorted(kw.items()))
    if key not in _cache:
        B, par = _batch(gpu_model.total_mass, which)
        par.update(kw)
        one, P = _solver(gpu_model, max_batch=NMAX, **par)
        two, _ = _solver(gpu_model, max_batch=NMAX, options={"fused_max": 0}, **par)
        ref = oracle.step(P, B["q"], B["v"], B["w_des"], B["vdot_des"], B["normals"], B["mu"], B["mask"])
        tr, dr = _traces(oracle, P, B)
        _cache[key] = (one, two, P, B, ref, tr, dr)
    return _cache[key]


def _check(torch, case, n, mats, skip_iters=()):
    one, two, P, B, ref = case[:5]
    assert one.plan_tick(n, want_mats=mats, want_pf=mats)["fused"] == 1 and two.plan_tick(n, want_mats=mats, want_pf=mats)["fused"] == 0
    Bn = {k: np.ascontiguousarray(v[:n]) for k, v in B.items()}
    got = _run_step(torch, one, Bn, "f64", want_mats=mats)
    alt = _run_step(torch, two, Bn, "f64", want_mats=mats)
    r = {k: ref[k][:n] for k in ("tau", "f", "status", "iters")}
    np.testing.assert_array_equal(got["status"], r["status"])
    ok = r["status"] == 0
    assert np.all(np.isfinite(got["tau"])) and np.all(np.isfinite(got["f"]))
    et, ef = elementwise_excess(got["tau"][ok], r["tau"][ok]), elementwise_excess(got["f"][ok], r["f"][ok])
    keep = np.ones(n, bool)
    keep[[i for i in skip_iters if i < n]] = False
    it_diff = float(np.mean(got["iters"][keep] != r["iters"][keep]))
    print("n=%d mats=%d: excess tau %.3g f %.3g, iters differing from the oracle %.3g, max iters %d" % (n, mats, et, ef, it_diff, got["iters"].max()))
    assert et <= 1.0 and ef <= 1.0, (et, ef)
    assert it_diff <= 2e-3, it_diff
    for k in ("f", "status", "iters") + (() if mats else ("tau",)):
        assert np.array_equal(got[k], alt[k]), (k, n, mats, "states that differ", np.unique(np.nonzero(np.asarray(got[k]).reshape(n, -1) != np.asarray(alt[k]).reshape(n, -1))[0]).tolist(),
                                                "max |diff|", float(np.abs(np.asarray(got[k], float) - alt[k]).max()))
    if mats:   # (with M, h, Jc the two-launch tick forms tau_partial in another recursion order: rounding only, tests/test_gpu_trip_skip.py)
        assert relerr(got["tau"], alt["tau"]) < 1e-9


def test_the_inputs_hold_every_situation(gpu_model, oracle):
    """CPU only (the solvers are built, nothing is launched): what the device tests below rely on"""
    st = _case(gpu_model, oracle, "standing")
    assert np.all(st[4]["status"] == 0) and st[4]["iters"].max() >= 4 and all(t.endswith("A") for t in st[5] if t)
    hard, trot = _case(gpu_model, oracle, "hard"), _case(gpu_model, oracle, "trot")
    for c in (hard, trot):
        assert np.all(c[4]["status"] == 0) and all(t.endswith("A") for t in c[5] if t)
    assert hard[4]["iters"].max() >= 10
    # partial steps among the four rows of N = 4, in the lone row of N = 17 and in every workgroup of N = 64
    tr = hard[5]
    assert any("P" in t for t in tr[:4]) and "P" in tr[16] and all(any("P" in t for t in tr[w:w + 16]) for w in range(0, NMAX, 16))
    # 2- and 3-foot stances, within the first 16 states already
    feet = lambda m: bin(int(m)).count("1")
    assert {2, 3} <= {feet(m) for m in trot[3]["mask"][:16]} and {2, 3, 4} <= {feet(m) for m in trot[3]["mask"]}
    assert any("P" in t for t in trot[5][:16])
    # drops that leave 0, 1 and 2 rows on their foot; two rows of one wavefront dropping in one trip
    # -- in the four rows of N = 4 already (hard), and among the 2- and 3-foot stances of N = 16 (trot)
    assert situations(hard[5], hard[6], 4) == ({"A", "P"}, {0, 1, 2}, True)
    assert situations(trot[5], trot[6], 16) == ({"A", "P"}, {0, 1, 2}, True)
    # dual-only trips: on the way to "infeasible"
    inf = _case(gpu_model, oracle, "infeasible")
    assert inf[4]["status"][16] == 2 and np.all(np.delete(inf[4]["status"], 16) == 0) and "D" in inf[5][16]
    lim = _case(gpu_model, oracle, "hard", max_iter=9)
    assert (lim[4]["status"][:17] == 1).any() and (lim[4]["status"] == 0).any() and set(lim[4]["status"]) <= {0, 1}


@pytest.mark.parametrize("mats", [True, False])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("which", ["standing", "hard", "trot"])
def test_chain_diet_tick(torch_cuda, gpu_model, oracle, which, n, mats):
    _check(torch_cuda, _case(gpu_model, oracle, which), n, mats)


@pytest.mark.parametrize("n", [17, 64])
def test_iteration_limit(torch_cuda, gpu_model, oracle, n):
    """max_iter = 9: most rows of the hard batch are stopped (status 1), some between a partial step and its full step; the rest finish"""
    case = _case(gpu_model, oracle, "hard", max_iter=9)
    _check(torch_cuda, case, n, True)
    _check(torch_cuda, case, n, False)


@pytest.mark.parametrize("n", [17, 64])
def test_infeasible_state(torch_cuda, gpu_model, oracle, n):
    """state 16 ends on a dual-only step that nothing blocks (status 2); its pivots on the way are degenerate, so its trip count is compared with the
    two-launch tick's only"""
    case = _case(gpu_model, oracle, "infeasible")
    _check(torch_cuda, case, n, True, skip_iters=(16,))
    _check(torch_cuda, case, n, False, skip_iters=(16,))
