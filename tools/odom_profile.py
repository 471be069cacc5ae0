#!/usr/bin/env python3
"""Time per launch of the base-estimate kernels beside the call they extend, for one rocprofv3 --kernel-trace --stats pass (the
program after `--`, no counters in the same run): 4 096 states, 5 warm-up + 30 launches of each call in turn -- the statistics come per kernel name:
    wbc_gait_estimated_batch        (gait_estimated_kernel): the yardstick; its device code is the parent commit's
    wbc_gait_estimated_odom_batch   (gait_estimated_odom_kernel), planes given
    wbc_base_estimate_batch         (base_estimate_kernel), planes given, q_est and v_est their own buffers (the copy rows are written)
usage: odom_profile.py [f64|f32] [N]
The contact, mask and odo words cycle through every trust pattern (tests/odom_ref.py's branch table); odo is restored before every launch by a copy,
which shows as its own row.  Needs the product library only."""
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
B = synth.make_batch(4, n, model.total_mass)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).T)).to(td).cuda()
ints = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
q, v, normals, f_prev = dev(B["q"]), dev(B["v"]), dev(B["normals"]), dev(B["f_prev"])
Jc = solver.dynamics(q, v, want=("M", "h", "Jc"))["Jc"]
r = dev(np.random.default_rng(0).uniform(-5.0, 5.0, (n, 18)))
cmd = dev(np.tile([0.3, 0.0, 0.1, -0.05], (n, 1)))
ph = torch.from_numpy(np.linspace(0.0, 1.0, n, endpoint=False)).to(td).cuda()   # every part of the cycle is present in every launch
i = np.arange(n)
trust = (i % 16).astype(np.int32)
odo0 = ints(np.where(trust == 7, 7, ((trust << 1) | (trust >> 3)) & 15))
contact0, mask0 = ints(trust), ints(trust | ((i // 16) % 16))
contact, mask, odo = contact0.clone(), mask0.clone(), odo0.clone()
events = torch.zeros(n, dtype=torch.int32, device="cuda")
swing = torch.zeros((36, n), dtype=td, device="cuda")
f_est = torch.zeros((12, n), dtype=td, device="cuda")
height = torch.zeros((4, n), dtype=td, device="cuda")
base = torch.cat([q[0:3], v[0:3]]).contiguous()
anchor = torch.zeros((12, n), dtype=td, device="cuda")
q_est, v_est = torch.empty_like(q), torch.empty_like(v)


def fresh(call):
    def go():
        contact.copy_(contact0); mask.copy_(mask0); odo.copy_(odo0)
        call()
    return go


calls = [fresh(lambda: solver.gait_estimated(q, v, cmd, Jc, r, f_prev, normals, contact, ph, mask, swing, events=events, f_est=f_est)),
         fresh(lambda: solver.gait_estimated_odom(q, v, cmd, Jc, r, f_prev, normals, contact, ph, mask, swing, base, anchor, odo, height=height,
                                                  q_est=q_est, v_est=v_est, events=events, f_est=f_est)),
         fresh(lambda: solver.base_estimate(q, v, contact, mask, base, anchor, odo, normals=normals, height=height, q_est=q_est, v_est=v_est))]
for call in calls:
    for rep in range(35):
        call()
torch.cuda.synchronize()
print("odom profile: %s, %d states, states with an anchored foot at the end: %d, base finite: %s"
      % (dtype, n, int(((odo & 15) != 0).sum()), bool(torch.isfinite(base).all())))
