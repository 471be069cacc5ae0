#!/usr/bin/env python3
"""Time per launch of the stiction kernels beside the ground plant's, for one rocprofv3 --kernel-trace --stats pass (the program after
`--`, no counters in the same run): 4 096 states, one scalar type per process, 5 warm-up + 30 rounds of three launches on the same states (the kernel
statistics count all 35 of each):
    wbc_integrate_ground_stick_batch (stick_integrate_kernel)   the law with the anchor spring + the plant step
    wbc_ground_stick_force_batch     (stick_force_kernel)       the law alone
    wbc_integrate_ground_batch       (ground_integrate_kernel)  the yardstick: the stateless plant of the same build, in the same visit
The feet of the batch straddle the ground as in tools/ground_profile.py; three quarters of the states come with their anchors set, 0 ... 2 mm from the
feet, so that unloaded, first-loaded, sticking and sliding feet are present in every wavefront.  q, v, anchor, stick are restored before EVERY launch
(the same four device copies, not timed by the kernel statistics), so that the three kernels start behind the same predecessor.
usage: stick_profile.py [f64|f32] [N]
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
B = synth.make_batch(3, n, model.total_mass)
dev = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).T)).to(td).cuda()
q0, v0 = dev(B["q"]), dev(B["v"])
normals, mu, tau = dev(B["normals"]), dev(B["mu"]), dev(B["tau_prev"])
d = solver.dynamics(q0, v0, want=("M", "h", "Jc", "pf"))
rng = np.random.default_rng(0)
height = d["pf"].reshape(4, 3, n)[:, 2, :].contiguous()                    # the ground at every foot's own height ...
height += torch.from_numpy(rng.uniform(-2e-3, 2e-3, (4, n))).to(td).cuda()   # ... +- 2 mm
anchor0 = d["pf"] + torch.from_numpy(rng.uniform(-2e-3, 2e-3, (12, n))).to(td).cuda()
stick0 = torch.from_numpy(np.where(np.arange(n) % 4 == 0, 0, 0b1111).astype(np.int32)).cuda()
q, v, anchor, stick = q0.clone(), v0.clone(), anchor0.clone(), stick0.clone()
f_gr = torch.zeros((12, n), dtype=td, device="cuda")
contact = torch.zeros(n, dtype=torch.int32, device="cuda")
seen = torch.zeros(n, dtype=torch.int32, device="cuda")
def restore():   # the same four device copies in front of every launch, so that the three kernels start behind the same predecessor
    q.copy_(q0); v.copy_(v0); anchor.copy_(anchor0); stick.copy_(stick0)


for rep in range(35):
    restore()
    solver.integrate_ground_stick(q, v, d["M"], d["h"], d["Jc"], tau, normals, height, mu, anchor, stick, f_gr=f_gr, contact=contact)
    seen.copy_(stick)
    restore()
    solver.integrate_ground(q, v, d["M"], d["h"], d["Jc"], tau, normals, height, mu, f_gr=f_gr, contact=contact)
    restore()
    solver.ground_stick_force(q, v, d["Jc"], normals, height, mu, anchor, stick, f_gr=f_gr, contact=contact)
torch.cuda.synchronize()
assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(v).all()) and bool(torch.isfinite(anchor).all())
frac = lambda w, sh: float(sum(((w >> (sh + k)) & 1).sum() for k in range(4))) / (4 * n)
print("%s, %d states, %s; feet in contact %.2f, loaded %.2f, slid %.2f" % (dtype, n, W.LIB_PATH, frac(contact, 0), frac(seen, 0), frac(seen, 4)))
