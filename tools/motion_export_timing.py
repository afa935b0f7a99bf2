"""Time the export of a recorded rollout at two stated sizes: 300 steps x 4096 envs and 300 steps x 64 envs of the 24-body humanoid, a random
recording (seed 77) with a reset every 60 .. 150 steps per env, form "motion" (pose_quat, pose_aa and trans_orig on).

    python tools/motion_export_timing.py            the kernel (HIP events around 20 back-to-back launches after 3 warm-up) and the whole
                                                    export_motion (segmentation, launch, copy to the host, the per-clip dict; 3 runs after 1 warm-up)
    python tools/motion_export_timing.py --cpu      the reference's own chain (render()'s conversion lines on scipy and poselib, frame by frame as
                                                    render() runs it, and _write_states_to_file once) on a SAMPLE of frames of the small recording,
                                                    on the host CPU, one process; extrapolated to both sizes and labelled as such
                                                    (tools/gen_golden_motion_export.py; needs the reference checkout and scipy)

Results: profiles/motion_export.txt."""
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

STEPS, SIZES, SEED, SAMPLE = 300, (4096, 64), 77, 256


def recording(envs, device="cpu"):
    """rb (T, N, 24, 13), dof_pos (T, N, 69), progress (T, N): unit quaternions, a reset every 60 .. 150 steps."""
    g = torch.Generator().manual_seed(SEED)
    rb = torch.randn(STEPS, envs, 24, 13, generator=g)
    rb[..., 3:7] /= rb[..., 3:7].norm(dim=-1, keepdim=True)
    dof = 0.5 * torch.randn(STEPS, envs, 69, generator=g)
    period = torch.randint(60, 151, (envs,), generator=g)
    phase = torch.randint(0, 150, (envs,), generator=g)
    progress = (torch.arange(STEPS)[:, None] + phase[None]) % period[None]
    return rb.to(device), dof.to(device), progress.to(device)


def cpu():
    import gen_golden_motion_export as GX
    rb, dof, progress = (t.numpy() for t in recording(SIZES[1]))
    pick = np.random.default_rng(SEED).choice(STEPS * SIZES[1], SAMPLE, replace=False)
    frames = rb.reshape(-1, 24, 13)[pick]
    GX.run_render(frames[:1, :, 3:7], frames[:1, 0, 0:3], np.float64)          # imports, TorchScript compilation
    t0 = time.perf_counter()
    for f in frames:                                                              # render() converts one frame per call (its assert on shape[0] == 1)
        GX.run_render(f[None, :, 3:7], f[None, 0, 0:3], np.float64)
    per_frame = (time.perf_counter() - t0) / SAMPLE
    t0 = time.perf_counter()
    GX.run_render(frames[:, :, 3:7], frames[:, 0, 0:3], np.float64)           # the same statements on the whole sample at once, which render() never does
    print(f"(the same statements on the {SAMPLE} frames in one batch: {(time.perf_counter() - t0) / SAMPLE * 1e6:.0f} us per frame)")
    t0 = time.perf_counter()
    dump = GX.run_write_states(rb, dof, progress, np.float64)
    whole_dump = time.perf_counter() - t0
    print(f"reference chain, host CPU, one process: render()'s conversion {per_frame * 1e6:.0f} us per frame on a sample of {SAMPLE} frames "
          f"(each call re-reads and compiles the statements: an upper bound); _write_states_to_file on {STEPS} x {SIZES[1]}: {whole_dump:.2f} s, {len(dump)} segments")
    for envs in SIZES:
        print(f"EXTRAPOLATED to {STEPS} x {envs} = {STEPS * envs} frames: conversion {per_frame * STEPS * envs:.1f} s, "
              f"dump {whole_dump * envs / SIZES[1]:.1f} s (linear in the env count)")


def gpu():
    from pulse_amd import kernels
    from pulse_amd.env import motion_export as ME
    dev = torch.device("cuda:0")
    trees = (syn.SMPL_PARENTS, torch.zeros(1, 24, 3))
    for envs in SIZES:
        rb, dof, progress = recording(envs, dev)
        seg = ME.segment_recording(progress)
        total = int(seg["frames"].sum())
        new = lambda *s: torch.empty(*s, device=dev)
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
            kernels.motion_export(new(total, 24, 4), new(total, 3), rb=rb, seg_env=seg["env"], seg_t0=seg["t0"], seg_frames=seg["frames"], parents=syn.SMPL_PARENTS,
                                  joint_map=syn.smpl_joint_map(), out_pose_quat=new(total, 24, 4), out_pose_aa=new(total, 72), out_trans_orig=new(total, 3))
        finally:
            kernels._launch = inner
        spanned, used, written = total * 24 * 52, total * (24 * 16 + 12), total * (2 * 24 * 16 + 72 * 4 + 24)
        print(f"pulse_motion_export, 20 back-to-back launches: {STEPS} x {envs}, {len(seg['keys'])} segments, {total} frames; {spanned / 1e6:.1f} MB of rb rows "
              f"spanned ({used / 1e6:.1f} MB used), {written / 1e6:.1f} MB written: {times[0]:.1f} us per launch ({(spanned + written) / times[0] / 1e3:.0f} GB/s over both)")
        whole = []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = ME.export_motion(rb, progress, trees, dof_pos=dof, fps=30)
            whole.append(time.perf_counter() - t0)
        print(f"export_motion whole (segmentation, launch, {written / 1e6:.1f} MB to the host, {len(out)} clip dicts): median {np.median(whole[1:]) * 1e3:.1f} ms")


if __name__ == "__main__":
    cpu() if sys.argv[1:] == ["--cpu"] else gpu()
