"""GPU: one timing of the crowd kernels (csrc/crowd_obs.hip) at 4096 envs, groups of 128, a 32 x 32 sensor on the synthetic height field,
beside pulse_traj_step's observation launch at the same size, alternated in one process.  A record (profiles/crowd_kernels.txt), not a gate.

    python tools/crowd_kernel_timing.py [out.txt]            event-timed windows (host enqueue included)
    python tools/crowd_kernel_timing.py --trace              200 calls of each and nothing else: the run to put under
                                                             rocprofv3 --kernel-trace --stats for the kernels' own times
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pulse_amd import ops, synthetic as syn
from pulse_amd._lib import TASK_OBS

dev = "cuda:0"
N, G, RES = 4096, 128, 32
P = RES * RES
g = syn.make_generator(11)
rb = syn.rigid_body_state(g, N)
spot = 6.0 + 14.0 * torch.rand(N, 1, 2, generator=g)                  # people spread over [6, 20] m of the field, bodies around their roots
rb[..., 0:2] = rb[..., 0:2] - rb[:, 0:1, 0:2] + spot
rb = rb.to(dev)
hs = syn.synthetic_height_field().to(dev)
rows, cols = hs.shape
hp, cp = syn.square_height_points(2.0, RES).to(dev), syn.center_height_points().to(dev)
head = syn.SMPL_BODY_NAMES.index("Head")
owner = torch.zeros(N // G, rows, cols, dtype=torch.int32, device=dev)
cells = torch.full((N, 200), -1, dtype=torch.int32, device=dev)
obs = torch.zeros(N, 20 + 3 * P + 165 + 3, device=dev)
verts = torch.zeros(N, 101, 3, device=dev)
verts[:, :, 0] = torch.linspace(0, 30, 101, device=dev)
progress = torch.zeros(N, dtype=torch.int64, device=dev)
traj = dict(what=TASK_OBS, dt=1 / 30, episode_dur=10.0, obs=obs)
sensor = dict(heightsamples=hs, height_points=hp, sensor_body=head, center_points=cp, use_center_height=True)
common = dict(sensor_body=head, center_points=cp, use_center_height=True, obs=obs, obs_offset=20)

calls = {
    "pulse_traj_step OBS, 32 x 32 heights (the plain task)": lambda: ops.traj_step(rb, verts, progress, **traj, **sensor),
    "pulse_traj_step OBS, no height sensor (crowd modes)": lambda: ops.traj_step(rb, verts, progress, **traj),
    "pulse_crowd_group_obs": lambda: ops.crowd_group_obs(rb, G, obs=obs, obs_offset=20 + 3 * P),
    "pulse_crowd_stamp (clear + stamp: two launches)": lambda: ops.crowd_stamp(rb, G, owner, cells),
    "pulse_crowd_heights, stamps": lambda: ops.crowd_heights(rb, hs, hp, group_size=G, owner=owner, **common),
    "pulse_crowd_heights, stamps + velocity_map": lambda: ops.crowd_heights(rb, hs, hp, group_size=G, owner=owner, velocity_map=True, **common),
    "pulse_crowd_heights, velocity_map, no groups": lambda: ops.crowd_heights(rb, hs, hp, velocity_map=True, **common),
}

if "--trace" in sys.argv:
    for f in calls.values():
        for _ in range(200):
            f()
    torch.cuda.synchronize()
    sys.exit(0)


def timed(f, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters                     # microseconds per call


for f in calls.values():
    for _ in range(200):
        f()
res = {k: [] for k in calls}
for rep in range(5):                                              # alternated: five windows of 1000 back-to-back calls each
    for k, f in calls.items():
        res[k].append(timed(f, 1000))

MB = 1e6
moved = [          # per launch, from the shapes: (kernel, requested reads, writes, note)
    ("pulse_traj_step OBS, heights", N * P * (8 + 4), N * (P + 20) * 4, "per sample: grid point 8 B, two int16 gathers; writes one float"),
    ("pulse_crowd_group_obs", N * (6 * G * 12 + 5 * 11 * 12 + 28), N * 165 * 4,
     "six passes over the group's G root positions (12 B, cache-resident after the first), 55 vectors of the 5 neighbours"),
    ("pulse_crowd_stamp", N * 200 * 28 + N * 200 * 4, 2 * N * 200 * 4 + N * 200 * 4,
     "clear: the cell list in, one int32 store per entry; stamp: root pose per point (cached), one atomicMax and one list entry out"),
    ("pulse_crowd_heights, stamps", N * P * (8 + 4 + 8), N * P * 4, "two int16 and two int32 (owner) gathers per sample"),
    ("pulse_crowd_heights, stamps + velocity_map", N * P * (8 + 4 + 8 + 12), N * P * 12, "plus the owner's velocity (12 B, where a cell is owned); three floats out"),
]
lines = [f"Crowd kernels, N = {N} envs, groups of {G} ({N // G} groups), {RES} x {RES} sensor, height field {rows} x {cols}, {torch.cuda.get_device_name(0)}",
         "microseconds per call, back-to-back launches on one stream (host enqueue of the Python wrapper included);",
         "five alternated windows of 1000 calls: min / median / max",
         ""]
for k, v in res.items():
    v = sorted(v)
    lines.append(f"{k:56s} {v[0]:8.2f} {v[2]:8.2f} {v[-1]:8.2f}")
lines += ["", "bytes per launch, derived from the shapes (reads as requested by the lanes: the gathers hit a field of "
          f"{rows * cols * 2 / MB:.2f} MB and an owner grid of {N // G * rows * cols * 4 / MB:.2f} MB, both cache-resident):"]
for k, rd, wr, note in moved:
    lines.append(f"{k:44s} reads {rd / MB:8.2f} MB  writes {wr / MB:8.2f} MB   ({note})")
text = "\n".join(lines) + "\n"
print(text)
out = [a for a in sys.argv[1:] if not a.startswith("--")]
if out:
    with open(out[0], "w") as fh:
        fh.write(text)
