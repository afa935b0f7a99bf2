"""GPU: one timing of the two launches the HumanoidAMP layer of the downstream tasks adds (env/humanoid_tasks.py, enable_amp_obs) at 4096
envs: the reference-state reset (pulse_task_ref_state_init, a quarter of the envs masked, every transform) and the per-step window launch
of a task env (pulse_amp_obs in history mode: shift + current frame + the finished window into a sink row).  A record
(profiles/task_amp.txt), not a gate.

    python tools/task_amp_timing.py [out.txt]            median of 20 event-timed calls after warm-up (host enqueue included)
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pulse_amd import ops, synthetic as syn
from pulse_amd.env.amp_window import AmpWindow
from pulse_amd.env.humanoid_tasks import SyntheticTaskSim
from pulse_amd.env.motion_lib import MotionLib

dev = "cuda:0"
N, S = 4096, 10
g = syn.make_generator(11)
lib = MotionLib.from_tables(syn.synthetic_motion_library(g, 1024), dev)
sim = SyntheticTaskSim(N, 2, dev, seed=3, dof_pos_bank=True)
ids = torch.randint(0, 1024, (N,), generator=g).to(dev)
times = (torch.rand(N, generator=g).to(dev) * lib.get_motion_length(ids)).contiguous()
mask = (torch.arange(N, device=dev) % 4 == 0)                       # a quarter of the envs
start, sampled = torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.int64, device=dev)
clears = tuple(torch.zeros(N, dtype=torch.int64, device=dev) for _ in range(3))
hs, cp = syn.synthetic_height_field().to(dev), syn.center_height_points().to(dev)
xy = (3.0 + torch.rand(N, 2, generator=g) * torch.tensor([20.0, 24.0])).to(dev)
win = AmpWindow({"numAMPObsSteps": S}, num_envs=N, device=dev, skeleton=syn.skeleton("smpl"), local_root_obs=True, upright=True, amp_obs_v=1)
sink = torch.zeros(N, win.num_obs() + 0, device=dev)


def reset(transform, **kw):
    return lambda: ops.task_ref_state_init(lib, ids, times, mask, sim.rigid_body_state, sim.dof_pos, sim.dof_vel, start, sampled, clears=clears,
                                           transform=transform, **kw)


def window():
    win.set_sink(sink)
    win.step(sim)


calls = {
    "pulse_task_ref_state_init NONE (traj)": reset("none"),
    "pulse_task_ref_state_init ZERO_XY (reach, strike)": reset("zero_xy"),
    "pulse_task_ref_state_init REMOVE_HEADING (speed)": reset("remove_heading"),
    "pulse_task_ref_state_init TERRAIN, 3 x 3 centre grid": reset("terrain", new_root_xy=xy, heightsamples=hs, center_points=cp),
    "pulse_amp_obs, history mode + sink (per step)": window,
}


def timed(f):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0                              # microseconds


res = {}
for k, f in calls.items():
    for _ in range(50):
        f()
    torch.cuda.synchronize()
    res[k] = sorted(timed(f) for _ in range(20))

J, W = 24, win.per_step
masked = int(mask.sum())
rec = lib.frame_stride * 4
MB = 1e6
moved = [   # per launch, from the shapes
    ("pulse_task_ref_state_init", N + masked * (2 * rec + 12), masked * (J * 13 + 2 * 3 * (J - 1)) * 4 + masked * (4 + 8 + 3 * 8),
     f"{N} mask flags; per masked env two frame records of {rec} B, id + time; writes {J} x 13 records, dof_pos, dof_vel, start time, id, three words"
     " (TERRAIN: + 8 B location, 18 int16 gathers from the cache-resident field)"),
    ("pulse_amp_obs, history mode + sink", N * ((J * 13 + 2 * 69) * 4 + (S - 1) * W * 4), N * S * W * 4 * 2,
     f"state of every env, the {S - 1} older frames of its window; writes the shifted window ({S} x {W} floats) and its copy in the sink row"),
]
lines = [f"Task AMP launches, N = {N} envs ({masked} masked for the reset), window {S} x {W}, motion library of 1024 clips, {torch.cuda.get_device_name(0)}",
         "microseconds per call, one event-timed call at a time after 50 warm-up calls (host enqueue of the Python wrapper included);",
         "20 calls: min / median / max", ""]
for k, v in res.items():
    lines.append(f"{k:56s} {v[0]:8.2f} {(v[9] + v[10]) / 2:8.2f} {v[-1]:8.2f}")
lines += ["", "bytes per launch, derived from the shapes:"]
for k, rd, wr, note in moved:
    lines.append(f"{k:40s} reads {rd / MB:8.2f} MB  writes {wr / MB:8.2f} MB   ({note})")
text = "\n".join(lines) + "\n"
print(text)
out = [a for a in sys.argv[1:] if not a.startswith("--")]
if out:
    with open(out[0], "w") as fh:
        fh.write(text)
