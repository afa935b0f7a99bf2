"""Time the evaluation sweep on one MI355X (profiles/eval_sweep.txt):

    python tools/bench_eval_sweep.py [--envs 4096] [--clips 2048] [--out FILE]

  * pulse_im_eval_accum alone at ``envs`` envs, 24 and 52 bodies: HIP events around 200 back-to-back launches after 20 warm-up launches;
  * IMAmpAgent.eval() over ``clips`` synthetic clips on ``envs`` envs (cfg2's network), host clock around the whole call (it ends
    synchronised: the results are read back), once with the accumulation kernel alone and once with ``return_positions=True`` -- the
    reference's path, which copies every env's body positions to the host on every step; each after one warm-up call.
Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pulse_amd import configs, ops  # noqa: E402
from pulse_amd.learning.im_amp import IMAmpAgent  # noqa: E402


def kernel_time(n, j, launches=200, warmup=20):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(j)
    rb = torch.randn(n, j, 13, generator=g).to(dev)
    ref = (rb[..., 0:3] + 0.05 * torch.randn(n, j, 3, generator=g).to(dev)).contiguous()
    ring, acc = ops.im_eval_state(n, j, dev)
    steps = torch.full((n,), 1 << 20, dtype=torch.int32, device=dev)
    for s in range(warmup):
        ops.im_eval_accum(rb, ref, steps, s, ring, acc)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for s in range(launches):
        ops.im_eval_accum(rb, ref, steps, warmup + s, ring, acc)
    b.record()
    torch.cuda.synchronize()
    assert torch.isfinite(acc).all() and int(acc[0, 5]) == warmup + launches
    return a.elapsed_time(b) * 1000.0 / launches


def sweep_time(envs, clips, humanoid="smpl"):
    cfg, _ = configs.agent_config("cfg2")
    vec_env, _ = configs.make_env(envs, cfg["horizon_length"], "cuda:0", seed=21, reference="motion_data", humanoid=humanoid, num_clips=clips,
                                  env_overrides={"auto_pmcp_soft": True})
    cfg.update({"vec_env": vec_env, "device": "cuda:0", "seed": 21, "train_dir": tempfile.mkdtemp()})
    ag = IMAmpAgent("pulse_amd", cfg)
    out = {}
    for name, kw in (("accum_kernel", {}), ("return_positions", {"return_positions": True})):
        ag.eval(**kw)                                   # warm-up: code objects, workspaces, the evaluation library's first load
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev = ag.eval(**kw)
        torch.cuda.synchronize()
        out[name] = {"seconds": time.perf_counter() - t0, "steps": sum(ev["batch_lengths"]), "batches": len(ev["batch_lengths"]),
                     "eval_mpjpe_all": ev["eval_mpjpe_all"], "eval_success_rate": ev["eval_success_rate"]}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_sweep needs a GPU")
    res = {"envs": args.envs, "clips": args.clips,
           "kernel_us_per_launch": {"smpl_24": kernel_time(args.envs, 24), "smplx_52": kernel_time(args.envs, 52)},
           "eval": sweep_time(args.envs, args.clips)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
