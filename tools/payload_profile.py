#!/usr/bin/env python3
"""The plant payload's cost, for one rocprofv3 --kernel-trace --stats pass: the same workload with and without a payload,
interleaved, so that rollout_kernel<..., PAYLOAD> / integrate_kernel<T, true> and their siblings appear side by side in the kernel stats.
usage: payload_profile.py rollout [N H]   -- persistent rollouts, fp64, observer on (default 1 024 x 20): 5 warm-up + 30 launches of each
       payload_profile.py integrate [N]   -- the per-tick forward dynamics after one tick, fp64 (default 8 192 states): 5 warm-up + 100 launches of each
       (add f32 as the last argument for the fp32 solver)
Payloads: 0 .. 8 kg, CoM offsets up to 0.15 m, every fifth state none.  Needs the product library only."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import wbc_quadruped_dob_amd as W   # noqa: E402
from wbc_quadruped_dob_amd import synth   # noqa: E402

argv = [a for a in sys.argv[1:] if a not in ("f32", "f64")]
dtype = "f32" if "f32" in sys.argv[1:] else "f64"
mode = argv[0]
n = int(argv[1]) if len(argv) > 1 else (1024 if mode == "rollout" else 8192)
H = int(argv[2]) if len(argv) > 2 else 20
obs = 1 if mode == "rollout" else 0
td = torch.float64 if dtype == "f64" else torch.float32
model = W.Model.from_urdf(W.SYNTHETIC_URDF)
solver = W.Solver(model, W.Params.from_dict(synth.default_params(observer_order=obs, dtype=dtype), dtype), dtype=dtype, device=0, max_batch=n)
B = synth.make_batch(2, n, model.total_mass)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).T)).to(td).cuda()
rng = np.random.default_rng(1)
m = rng.uniform(0.0, 8.0, n)
m[::5] = 0.0
c = rng.uniform(-0.15, 0.15, (n, 3))
I = np.stack([np.diag(rng.uniform(0.2, 1.0, 3) * mi * 0.01) for mi in m])
pay = W.payload_rows(m, c, I).astype(np.float64)
pay = torch.from_numpy(np.ascontiguousarray(pay)).to(td).cuda()
q0, v0 = dev(B["q"]), dev(B["v"])
q, v = q0.clone(), v0.clone()
mask = torch.from_numpy(B["mask"]).cuda()
args = [dev(B[k]) for k in ("w_des", "vdot_des", "normals", "mu")]
if mode == "rollout":
    ig0 = solver.dynamics(q0, v0, want=("p",))["p"].clone()   # the observer's integral starts at the momentum
    ig, rr = ig0.clone(), torch.zeros((18, n), dtype=td, device="cuda")
    out = solver.step(q, v, *args, mask, dev(B["tau_prev"]), dev(B["f_prev"]), obs_integ=ig, obs_r=rr, want_mats=True)
    out["iters"] = torch.zeros(n, dtype=torch.int32, device="cuda")
    out["pf"] = solver.empty(12, n)
    tau0, f0 = out["tau"].clone(), out["f"].clone()
    for rep in range(35):
        for p in (None, pay):
            q.copy_(q0); v.copy_(v0); ig.copy_(ig0); rr.zero_(); out["tau"].copy_(tau0); out["f"].copy_(f0)
            solver.rollout(H, q, v, *args, mask, out, ig, rr, payload=p)
else:
    out = solver.step(q, v, *args, mask, dev(B["tau_prev"]), dev(B["f_prev"]), want_mats=True)
    for rep in range(105):
        for p in (None, pay):
            q.copy_(q0); v.copy_(v0)
            solver.integrate(q, v, out["M"], out["h"], out["Jc"], out["tau"], out["f"], payload=p)
torch.cuda.synchronize()
print("ok", mode, dtype, n, H if mode == "rollout" else "")
