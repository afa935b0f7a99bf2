"""pulse_keypoint_push: the error table and the launch, event-timed (profiles/keypoint_stream.txt).  A record, no threshold.

    python tools/keypoint_stream_timing.py [--cpu] [--out FILE]

  * the kernel's worst error per field on the fixture's two streams beside err_pos / err_vel, the reference's own fp32 error (what
    tests/test_keypoint_stream_gpu.py asserts at 4 x);
  * the launch at N = 64, 1024 and 4096 envs with a full history (H = 30 pushes first): HIP events around 20 back-to-back launches after 3 warm-up
    launches, with the bytes the algorithm moves per launch and their share of 8 TB/s;
  * --cpu: for scale, the reference's per-step statements on the host at the same sizes -- humanoid_im_mcp_demo.py:255-290 RESTATED with the same
    numpy / scipy calls (the reference tree is not needed): reorder, limb scale, three deque(maxlen=30) appends, three gaussian_filter1d over the
    whole history, the frame product and the finite difference in torch.  The HTTP fetch and the upload are left out.
"""
import argparse
import collections
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from pulse_amd import kernels  # noqa: E402
from pulse_amd import synthetic as syn  # noqa: E402
from pulse_amd.env.keypoint_stream import KeypointStream  # noqa: E402

SIZES = (64, 1024, 4096)
H, J, REPS, WARM = 30, 24, 20, 3
HBM_BYTES_PER_S = 8.0e12


def bytes_per_launch(n, h=H, j=J):
    """What one push moves with a full history: keypoints, count, prev_pos and h - 1 ring slots read; one ring slot, pos, vel, prev_pos, raw and
    count written (the tap table, 3 h floats per launch, stays in cache)."""
    read = n * (12 * j + 4 + 12 * j + (h - 1) * 12 * (j + 1))
    written = n * (12 * (j + 1) + 4 * 12 * j + 4)
    return read + written


def frames(n, count, seed=0):
    g = torch.Generator().manual_seed(seed)
    root = torch.cumsum(0.02 * torch.randn(count, n, 1, 3, generator=g), 0)
    return (root + 0.3 * torch.randn(1, n, J, 3, generator=g) + 0.01 * torch.randn(count, n, J, 3, generator=g)).float()


def error_table(dev, say):
    import gen_golden_keypoint_stream as GK
    fx = GK.load()
    for name, (count, history) in GK.STREAMS.items():
        s = KeypointStream(GK.N, dev, history=history)
        wp = wv = 0.0
        for t in range(count):
            s.push(torch.from_numpy(fx[f"j3d_{name}"][t]).to(dev))
            wp = max(wp, float(np.abs(s.pos.cpu().numpy() - fx[f"pos64_{name}"][t]).max()))
            wv = max(wv, float(np.abs(s.vel.cpu().numpy() - fx[f"vel64_{name}"][t]).max()))
        ep, ev = float(fx["err_pos"]), float(fx["err_vel"])
        say(f"stream {name} ({count} frames, history {history}): pos {wp:.3e} = {wp / ep:.2f} x err_pos ({ep:.3e}); vel {wv:.3e} = {wv / ev:.2f} x err_vel ({ev:.3e})")


def time_launch(dev, n, say):
    s = KeypointStream(n, dev, history=H)
    f = frames(n, H + WARM + REPS).to(dev)
    for t in range(H + WARM):
        s.push(f[t])
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for t in range(H + WARM, H + WARM + REPS):
        s.push(f[t])
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) * 1e3 / REPS
    nbytes = bytes_per_launch(n)
    say(f"N = {n:5d}: {us:8.2f} us per launch ({REPS} back-to-back after {WARM} warm-up, full history {H}); {nbytes / 1e6:8.3f} MB moved = "
        f"{nbytes / (us * 1e-6) / 1e9:8.1f} GB/s = {100 * nbytes / (us * 1e-6) / HBM_BYTES_PER_S:5.2f} % of 8 TB/s")


def time_host(n, say):
    from scipy.ndimage import gaussian_filter1d
    jm, parents = syn.smpl_joint_map(), syn.SMPL_PARENTS
    mean = np.array(kernels.KEYPOINT_MEAN_LIMB_LENGTHS, dtype=np.float32)[None, :]
    mat = torch.from_numpy(kernels.keypoint_frame("y_up")).float()
    f = frames(n, H + REPS).numpy().astype(np.float64)
    root_acc, body_acc, prev = collections.deque(maxlen=H), collections.deque(maxlen=H), torch.zeros(n, J, 3)
    t0 = None
    for t in range(H + REPS):
        if t == H:
            t0 = time.perf_counter()
        p = f[t][:, jm]
        trans = p[:, [0]]
        p = p - trans
        limb = np.array([np.linalg.norm(p[:, parents[i]] - p[:, i], axis=-1) for i in range(1, 6)]).transpose(1, 0)
        p /= (limb / mean).mean(axis=-1)[:, None, None]
        root_acc.append(trans)
        r = np.array(root_acc)
        r[..., 2] = gaussian_filter1d(r[..., 2], 10, axis=0, mode="mirror")
        r[..., :2] = gaussian_filter1d(r[..., :2], 5, axis=0, mode="mirror")
        body_acc.append(p)
        b = gaussian_filter1d(np.array(body_acc), 2, axis=0, mode="mirror")[-1]
        pos = torch.from_numpy(b + r[-1]).float().matmul(mat.T)
        vel = torch.from_numpy(np.gradient(torch.stack([prev, pos], dim=1).numpy(), axis=-3) / (1 / 30))[:, 0]
        prev = pos
    us = (time.perf_counter() - t0) * 1e6 / REPS
    say(f"N = {n:5d}: {us:10.1f} us per step on the host (numpy / scipy / torch-CPU restatement of lines 255-290, full history, {REPS} steps; vel {tuple(vel.shape)})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    if not torch.cuda.is_available():
        raise SystemExit("keypoint_stream_timing: needs a GPU (no fallback)")
    dev = torch.device("cuda:0")
    say(f"pulse_keypoint_push on {torch.cuda.get_device_name(0)}")
    say("-- error on the fixture's streams (fp64 model; err = the reference's own fp32 error)")
    error_table(dev, say)
    say("-- the launch, HIP events")
    for n in SIZES:
        time_launch(dev, n, say)
    if a.cpu:
        say("-- the reference's per-step host statements, for scale")
        for n in SIZES:
            time_host(n, say)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
