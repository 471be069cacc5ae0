#!/usr/bin/env python3
"""The cost of scoring a rollout, for one rocprofv3 --kernel-trace --stats pass: the same persistent rollouts scored and
unscored, interleaved, so that rollout_scored_kernel and its sibling rollout_kernel<..., WARM = true> appear side by side in the kernel
stats; then the selection kernel at G x K = 16 x 64 and 1 x 1024.
usage: score_profile.py [N H] [f32] [per_tick]   -- default 1 024 x 20, fp64, observer on: 5 warm-up + 30 launches of each
       per_tick: rollout_persistent = 0 (score_tick_kernel behind every tick's integrate launch)
Needs the product library only."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import wbc_quadruped_dob_amd as W   # noqa: E402
from wbc_quadruped_dob_amd import synth   # noqa: E402

flags = ("f32", "f64", "per_tick")
argv = [a for a in sys.argv[1:] if a not in flags]
dtype = "f32" if "f32" in sys.argv[1:] else "f64"
n = int(argv[0]) if len(argv) > 0 else 1024
H = int(argv[1]) if len(argv) > 1 else 20
td = torch.float64 if dtype == "f64" else torch.float32
model = W.Model.from_urdf(W.SYNTHETIC_URDF)
opts = {"rollout_persistent": 0} if "per_tick" in sys.argv[1:] else {}
solver = W.Solver(model, W.Params.from_dict(synth.default_params(observer_order=1, dtype=dtype), dtype), dtype=dtype, device=0, max_batch=n, options=opts)
solver.set_score_params(dict(w_tau=1e-3, w_f=1e-4, w_pos=5.0, w_rot=2.0, w_vel=0.5, w_omega=0.5, w_q=0.2, w_qd=0.02, terminal=5.0))
B = synth.make_batch(2, n, model.total_mass)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).T)).to(td).cuda()
goal = np.zeros((n, 10))
goal[:, 0:3] = B["q"][:, 0:3] + 0.1
goal[:, 3:7] = B["q"][:, 3:7]
goal = dev(goal)
q0, v0 = dev(B["q"]), dev(B["v"])
q, v = q0.clone(), v0.clone()
mask = torch.from_numpy(B["mask"]).cuda()
w_des, vdot_des, normals, mu = (dev(B[k]) for k in ("w_des", "vdot_des", "normals", "mu"))
ig0 = solver.dynamics(q0, v0, want=("p",))["p"].clone()   # the observer's integral starts at the momentum
ig, rr = ig0.clone(), torch.zeros((18, n), dtype=td, device="cuda")
out = solver.step(q, v, w_des, vdot_des, normals, mu, mask, dev(B["tau_prev"]), dev(B["f_prev"]), obs_integ=ig, obs_r=rr, want_mats=True)
out["iters"] = torch.zeros(n, dtype=torch.int32, device="cuda")
out["pf"] = solver.empty(12, n)
tau0, f0 = out["tau"].clone(), out["f"].clone()
cost = torch.zeros(n, dtype=td, device="cuda")
for rep in range(35):
    for scored in (False, True):
        q.copy_(q0); v.copy_(v0); ig.copy_(ig0); rr.zero_(); out["tau"].copy_(tau0); out["f"].copy_(f0)
        if scored:
            solver.rollout_scored(H, q, v, normals, mu, mask, out, w_des, vdot_des, goal, cost, obs_integ=ig, obs_r=rr)
        else:
            solver.rollout(H, q, v, w_des, vdot_des, normals, mu, mask, out, ig, rr)
c1024 = torch.rand(1024, dtype=td, device="cuda") * 10
for rep in range(35):
    W.select_rollouts(c1024, 64, 0.5, want_weights=True)
    W.select_rollouts(c1024, 1024, 0.5, want_weights=True)
torch.cuda.synchronize()
print("ok", dtype, n, H, "per_tick" if opts else "persistent", "mean cost %.6g" % float(cost.mean()))
