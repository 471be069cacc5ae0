#!/usr/bin/env python3
"""Time per launch of the command-driven reference kernels beside the plan-driven calls they stand in for, for one rocprofv3
--kernel-trace --stats pass (the program after `--`, no counters in the same run): 4 096 states, 5 warm-up + 30 launches of each call in turn -- the
statistics come per kernel name:
    wbc_reference_batch             (com_reference_kernel): the yardstick; its device code is the parent commit's
    wbc_reference_swing_batch       (com_swing_reference_kernel): likewise
    wbc_reference_cmd_batch         (cmd_reference_kernel), com and ref written
    wbc_reference_cmd_swing_batch   (cmd_swing_reference_kernel), com, ref and foot written
usage: cmdref_profile.py [f64|f32] [N]
The states, masks and plans are tests-free: synth.make_batch's, every mask pattern, plans around the feet's nominal height; the planes are level ground
with a per-foot ripple, a sixteenth of the states reset in every launch; trunk is restored before every launch by a copy, which shows as its own
row.  Needs the product library only."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import wbc_quadruped_dob_amd as W   # noqa: E402
from wbc_quadruped_dob_amd import synth   # noqa: E402

dtype = next((a for a in sys.argv[1:] if a in ("f64", "f32")), "f64")
n = int(next((a for a in sys.argv[1:] if a.isdigit()), 4096))
td = torch.float64 if dtype == "f64" else torch.float32
model = W.Model.from_urdf(W.SYNTHETIC_URDF)
solver = W.Solver(model, W.Params.from_dict(synth.default_params(dtype=dtype), dtype), dtype=dtype, device=0, max_batch=n)
solver.set_ref_params(synth.default_ref_params())
B = synth.make_batch(4, n, model.total_mass)
rng = np.random.default_rng(0)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).T)).to(td).cuda()
ints = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
q, v = dev(B["q"]), dev(B["v"])
plan = dev(synth.make_plan(B))
i = np.arange(n)
mask = ints(i % 16)
swing = np.zeros((n, 36))
for k in range(4):
    p0 = B["q"][:, 0:3] + rng.uniform(-0.3, 0.3, (n, 3)) - np.array([0.0, 0.0, 0.4])
    swing[:, 9 * k:9 * k + 3], swing[:, 9 * k + 3:9 * k + 6] = p0, p0 + rng.uniform(-0.1, 0.1, (n, 3))
    swing[:, 9 * k + 6], swing[:, 9 * k + 7], swing[:, 9 * k + 8] = 0.05, 0.25, rng.uniform(0.0, 0.2, n)
swing = dev(swing)
cmd = dev(np.tile([0.3, 0.05, 0.5, -0.05], (n, 1)))
g = rng.uniform(-0.05, 0.05, (n, 4, 2))
nrm = np.concatenate([-g, np.ones((n, 4, 1))], 2) / np.sqrt((g * g).sum(2) + 1.0)[:, :, None]
normals = dev(nrm.reshape(n, 12))
height = dev(nrm[:, :, 2] * (B["q"][:, 2:3] - 0.4))
reset = ints((i % 16 == 0).astype(np.int32))
trunk0 = dev(np.concatenate([B["q"][:, 0:2], rng.uniform(-3.0, 3.0, (n, 1)), B["q"][:, 2:3] - 0.4, np.zeros((n, 2))], 1))
trunk = trunk0.clone()
out_plan, out_cmd = {}, {}


def fresh(call):
    def go():
        trunk.copy_(trunk0)
        call()
    return go


calls = [lambda: solver.reference(q, v, plan, 0.1, out=out_plan, want_com=True),
         lambda: solver.reference_swing(q, v, plan, mask, swing, 0.0, out=out_plan, want_com=True, want_foot=True),
         fresh(lambda: solver.reference_cmd(q, v, cmd, normals, height, trunk, reset=reset, out=out_cmd, want_com=True, want_ref=True)),
         fresh(lambda: solver.reference_cmd_swing(q, v, cmd, normals, height, trunk, mask, swing, reset=reset, out=out_cmd, want_com=True, want_ref=True,
                                                  want_foot=True))]
for call in calls:
    for rep in range(35):
        call()
torch.cuda.synchronize()
print("cmdref profile: %s, %d states, trunk moved: %s, outputs finite: %s"
      % (dtype, n, bool((trunk != trunk0).any()), bool(torch.isfinite(out_cmd["w_des"]).all() and torch.isfinite(trunk).all())))
