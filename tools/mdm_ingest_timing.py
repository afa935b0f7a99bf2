"""Time the conversion of generated (text-to-motion) clips at two stated sizes: the fixture (tests/golden/mdm_ingest.npz: 4 clips, 112 frames) and
a workload of 4096 clips of 196 frames, the length MDM emits (64 clips of synthetic.synthetic_mdm_result, seed 77, jitter 1, tiled 64 times).

    python tools/mdm_ingest_timing.py            each entry point (HIP events around 20 back-to-back calls after 3 warm-up): pulse_motion_euler_pose
                                                 (one launch), pulse_motion_ingest (one), pulse_motion_smooth (three); and MotionLib.from_mdm_data whole
                                                 on the 64 clips (median of 5 after 1 warm-up)
    python tools/mdm_ingest_timing.py --cpu      the reference script's own statements for the 64 clips on the host CPU, one process
                                                 (tools/gen_golden_mdm_ingest.py:run_reference in fp64; needs the reference checkout and scipy)

Results: profiles/mdm_ingest.txt."""
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

BASE, TILES, FRAMES, SEED = 64, 64, 196, 77


def clips():
    return syn.synthetic_mdm_result(syn.make_generator(SEED), BASE, frames=FRAMES, jitter=1.0, num_slots=BASE)


def cpu():
    import gen_golden_mdm_ingest as GM
    result, _ = clips()
    run = lambda i: GM.run_reference({"thetas": result["thetas"][i], "root_translation": result["root_translation"][i]}, np.float64)
    run(0)                                                      # imports, TorchScript compilation
    t0 = time.perf_counter()
    for i in range(BASE):
        run(i)
    dt = time.perf_counter() - t0
    print(f"reference statements, host CPU, one process, fp64: {BASE} clips, {BASE * FRAMES} frames: {dt:.2f} s ({dt / (BASE * FRAMES) * 1e6:.1f} us per frame, "
          f"{dt / BASE * 4096:.0f} s for 4096 clips at that rate); quat_correct is the stand-in's Python loop")


def timed_entries(dev, theta, raw, frames, trees, label):
    from pulse_amd import kernels
    total = int(frames.sum())
    pose, trans = torch.empty_like(theta), torch.empty_like(raw)
    ing_rot, ing_trans = torch.empty(total, 24, 4, device=dev), torch.empty(total, 3, device=dev)
    out = {"rot": torch.empty(total, 24, 4, device=dev), "trans": torch.empty(total, 3, device=dev), "pq": torch.empty(total, 24, 4, device=dev),
           "aa": torch.empty(total, 72, device=dev), "orig": torch.empty(total, 3, device=dev)}
    inner, times = kernels._launch, {}

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
        times[name] = e0.elapsed_time(e1) * 1e3 / 20

    kernels._launch = timed
    try:
        kernels.motion_euler_pose(pose, trans, src_theta=theta, src_trans=raw, clip_frames=frames)
        kernels.motion_ingest(ing_rot, ing_trans, src_pose=pose, src_trans=trans, clip_src_start=torch.cumsum(frames, 0) - frames, clip_skip=torch.ones_like(frames),
                              clip_frames=frames, parents=trees[0], joint_map=syn.smpl_joint_map(), mirror_map=syn.mirror_body_map(), out_pose_aa=out["aa"],
                              out_trans_orig=out["orig"])
        kernels.motion_smooth(out["rot"], out["trans"], in_rot=ing_rot, in_trans=ing_trans, clip_frames=frames, parents=trees[0], out_pose_quat=out["pq"])
    finally:
        kernels._launch = inner
    # compulsory traffic per frame: euler 300 in + 300 out; smooth: bits 16 J in + 4 out, scan 4 + 4, filter 16 J + 12 + 4 in, 32 J + 12 out
    moved = {"pulse_motion_euler_pose": total * 600, "pulse_motion_ingest": total * (300 + 16 * 24 + 12 + 288 + 12),
             "pulse_motion_smooth": total * (16 * 24 + 4 + 8 + 16 * 24 + 16 + 32 * 24 + 12)}
    print(f"{label}: {frames.numel()} clips, {total} frames")
    for name, us in times.items():
        print(f"  {name:26s} {us:9.1f} us per call   {moved[name] / 1e6:9.2f} MB compulsory   {moved[name] / us / 1e3:7.0f} GB/s")


def gpu():
    import gen_golden_mdm_ingest as GM
    from pulse_amd.env.motion_lib import MotionLib
    dev = torch.device("cuda:0")
    fx = GM.load()
    fc = GM.clips_of(fx)
    trees = (list(syn.SMPL_PARENTS), torch.zeros(1, 24, 3))
    timed_entries(dev, torch.from_numpy(np.concatenate([c["thetas"].reshape(-1, 72) for c in fc])).to(dev),
                  torch.from_numpy(np.concatenate([c["root_translation"] for c in fc])).to(dev), torch.tensor([len(c["thetas"]) for c in fc]), trees, "fixture")
    result, trees = clips()
    theta = torch.from_numpy(np.concatenate([t.reshape(-1, 72) for t in result["thetas"]])).to(dev).repeat(TILES, 1)
    raw = torch.from_numpy(np.concatenate(result["root_translation"])).to(dev).repeat(TILES, 1)
    timed_entries(dev, theta, raw, torch.full((BASE * TILES,), FRAMES, dtype=torch.int64), trees, "workload")
    whole = []
    for i in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        MotionLib.from_mdm_data(result, trees, device=dev, generator=torch.Generator().manual_seed(i))
        torch.cuda.synchronize()
        whole.append(time.perf_counter() - t0)
    print(f"MotionLib.from_mdm_data whole on {BASE} clips of {FRAMES} frames (host planning, staging, five launches, first load_motions): median {np.median(whole[1:]) * 1e3:.1f} ms")


if __name__ == "__main__":
    cpu() if sys.argv[1:] == ["--cpu"] else gpu()
