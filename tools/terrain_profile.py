#!/usr/bin/env python3
"""Time per launch of the terrain kernels, for one rocprofv3 --kernel-trace --stats pass (the program after `--`, no counters in the
same run): 4 096 states on four rippled 64 x 48 tiles laid under the batch, 5 warm-up + 30 launches of each call in turn -- the statistics come
per kernel name:
    wbc_terrain_sample_batch          (terrain_sample_kernel), 4 096 points = the states' base x, y; z, n, d all written
    wbc_terrain_feet_batch            (terrain_feet_kernel), mask and swing given, surf written
    wbc_gait_terrain_batch            (gait_terrain_kernel), a trot in full swing, surf written
    wbc_gait_estimated_terrain_batch  (gait_estimated_terrain_kernel), f_est and surf written
    wbc_gait_batch, wbc_gait_estimated_batch  (gait_kernel, gait_estimated_kernel) on the same states -- the yardsticks: what the walking tick paid
                                      for its first launch before
usage: terrain_profile.py [f64|f32] [N]
Needs the product library only."""
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
q, v, normals, f_prev = dev(B["q"]), dev(B["v"]), dev(B["normals"]), dev(B["f_prev"])
Jc = solver.dynamics(q, v, want=("M", "h", "Jc"))["Jc"]
r = dev(np.random.default_rng(0).uniform(-5.0, 5.0, (n, 18)))
contact = torch.zeros(n, dtype=torch.int32, device="cuda")
cmd = dev(np.tile([0.3, 0.0, 0.1, -0.05], (n, 1)))
ph = torch.from_numpy(np.linspace(0.0, 1.0, n, endpoint=False)).to(td).cuda()   # every part of the cycle is present in every launch
mask = torch.full((n,), 0b1111, dtype=torch.int32, device="cuda")
events = torch.zeros(n, dtype=torch.int32, device="cuda")
swing = torch.zeros((36, n), dtype=td, device="cuda")
f_est = torch.zeros((12, n), dtype=td, device="cuda")
# the terrain: tile t = 0.05 x + 0.006 sin(2 pi (x / 0.125 + t / 4)) cos(2 pi y / 0.25) on 64 x 48 nodes, cell 2^-6, centred under the batch
cell, nx, ny = 2.0 ** -6, 64, 48
x0, y0 = float(B["q"][:, 0].mean()) - 0.5 * (nx - 1) * cell, float(B["q"][:, 1].mean()) - 0.5 * (ny - 1) * cell
X, Y = np.meshgrid(x0 + cell * np.arange(nx), y0 + cell * np.arange(ny))
z = np.stack([0.05 * X + 0.006 * np.sin(2 * np.pi * (X / 0.125 + t / 4.0)) * np.cos(2 * np.pi * Y / 0.25) for t in range(4)])
terrain = W.Terrain(torch.from_numpy(z).to(td).cuda().contiguous(), x0, y0, cell, (torch.arange(n, dtype=torch.int32) % 4).cuda())
xy = q[0:2].contiguous()
planes = dict(height=torch.zeros((4, n), dtype=td, device="cuda"), surf=torch.zeros((4, n), dtype=td, device="cuda"))
nrm = normals.clone()
calls = [lambda: solver.gait_terrain(terrain, q, v, cmd, ph, mask, swing, contact=contact, events=events, normals=nrm, **planes),
         lambda: solver.gait_estimated_terrain(terrain, q, v, cmd, Jc, r, f_prev, nrm, contact, ph, mask, swing, events=events, f_est=f_est, **planes),
         lambda: solver.terrain_feet(terrain, q, mask=mask, swing=swing, normals=nrm, **planes),      # (behind the gait calls: feet are in the air)
         lambda: solver.terrain_sample(terrain, xy),
         lambda: solver.gait(q, v, cmd, ph, mask, swing, contact=contact, events=events),
         lambda: solver.gait_estimated(q, v, cmd, Jc, r, f_prev, normals, contact, ph, mask, swing, events=events, f_est=f_est)]
for call in calls:
    for rep in range(35):
        call()
torch.cuda.synchronize()
print("terrain profile: %s, %d states, %s" % (dtype, n, W.LIB_PATH))
