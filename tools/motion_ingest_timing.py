"""Time the conversion of raw SMPL clips at one stated size: 256 synthetic clips of 45 .. 180 converted frames at 30 / 60 / 120 Hz
(synthetic.synthetic_smpl_data, seed 77), every optional output on.

    python tools/motion_ingest_timing.py            the kernel (HIP events around 20 back-to-back launches after 3 warm-up) and the whole
                                                    MotionLib.from_smpl_data (staging, launch, first load_motions; 5 runs after 1 warm-up)
    python tools/motion_ingest_timing.py --cpu      the reference's own statements for the same clips on the host CPU, one process
                                                    (tools/gen_golden_motion_ingest.py:run_reference in fp64; needs the reference checkout and scipy)

Results: profiles/motion_ingest.txt."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from pulse_amd import synthetic as syn  # noqa: E402

CLIPS, SEED = 256, 77


def clips():
    return syn.synthetic_smpl_data(syn.make_generator(SEED), CLIPS, framerate=[(30, 60, 120)[c % 3] for c in range(CLIPS)], num_slots=CLIPS)


def cpu():
    import gen_golden_motion_ingest as GI
    data, _ = clips()
    run = lambda e: GI.run_reference({"poses": e["poses"], "trans": e["trans"], "framerate": float(e["mocap_framerate"]), "bound": 0}, np.float64)
    first = next(iter(data.values()))
    run(first)                                                  # imports, TorchScript compilation
    frames, t0 = 0, time.perf_counter()
    for e in data.values():
        frames += run(e)[1]["pose_aa"].shape[0]
    dt = time.perf_counter() - t0
    print(f"reference statements, host CPU, one process: {CLIPS} clips, {frames} converted frames: {dt:.2f} s ({dt / frames * 1e6:.1f} us per frame); "
          "both scripts run per clip, the isaac one twice over (double)")


def gpu():
    from pulse_amd import kernels
    from pulse_amd.env.motion_lib import MotionLib, plan_smpl_clips
    dev = torch.device("cuda:0")
    data, trees = clips()
    plan, _ = plan_smpl_clips(data)
    raw = torch.tensor([c["raw_frames"] for c in plan], dtype=torch.int64)
    frames = torch.tensor([c["frames"] for c in plan], dtype=torch.int64)
    total, staged = int(frames.sum()), int(raw.sum())
    pose = torch.cat([torch.from_numpy(data[c["key"]]["poses"]) for c in plan]).to(dev)
    trans = torch.cat([torch.from_numpy(data[c["key"]]["trans"]) for c in plan]).to(dev)
    out = {"rot": torch.empty(total, 24, 4, device=dev), "trans": torch.empty(total, 3, device=dev), "pq": torch.empty(total, 24, 4, device=dev),
           "aa": torch.empty(total, 72, device=dev), "orig": torch.empty(total, 3, device=dev)}
    args = dict(src_pose=pose, src_trans=trans, clip_src_start=torch.cumsum(raw, 0) - raw, clip_skip=torch.tensor([c["skip"] for c in plan], dtype=torch.int64),
                clip_frames=frames, parents=trees[0], joint_map=syn.smpl_joint_map(), mirror_map=syn.mirror_body_map(), out_pose_quat=out["pq"],
                out_pose_aa=out["aa"], out_trans_orig=out["orig"])
    # the launch alone: the wrapper's own launch is replaced by 3 warm-up and 20 timed launches of the struct it built (its clip tables stay alive)
    inner, times = kernels._launch, []

    def timed(name, a):
        for _ in range(3):
            inner(name, a)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            inner(name, a)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3 / 20)

    kernels._launch = timed
    try:
        kernels.motion_ingest(out["rot"], out["trans"], **args)
    finally:
        kernels._launch = inner
    nbytes = total * (72 * 4 + 12) + total * (2 * 24 * 16 + 72 * 4 + 24)
    print(f"pulse_motion_ingest, 20 back-to-back launches: {CLIPS} clips, {staged} staged -> {total} converted frames, {nbytes / 1e6:.2f} MB to move: "
          f"{times[0]:.1f} us per launch ({nbytes / times[0] / 1e3:.0f} GB/s)")
    whole = []
    for i in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        MotionLib.from_smpl_data(data, trees, device=dev, generator=torch.Generator().manual_seed(i))
        torch.cuda.synchronize()
        whole.append(time.perf_counter() - t0)
    print(f"MotionLib.from_smpl_data whole (host planning, staging {staged} raw frames, ingest, first load_motions): median {np.median(whole[1:]) * 1e3:.1f} ms")


if __name__ == "__main__":
    cpu() if sys.argv[1:] == ["--cpu"] else gpu()
