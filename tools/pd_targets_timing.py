"""GPU: one timing of the actuation launch (csrc/pd_targets.hip) beside the two eager ops it replaces -- the wrapper's torch.clamp and the task's
torch.addcmul -- and, for res_action, beside the eager chain (seven launches with the clamp), alternated in one process.  A record
(profiles/pd_targets.txt), not a gate.

    python tools/pd_targets_timing.py [out.txt]         event-timed windows of back-to-back calls (host enqueue included)
    python tools/pd_targets_timing.py --trace           200 calls of each form at 4096 x 69 and nothing else: the run to put under
                                                        rocprofv3 --kernel-trace --stats for the kernels' own times (tools/rocprof_summary.py)
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pulse_amd import ops

dev = "cuda:0"
g = torch.Generator().manual_seed(0)
TRACE = "--trace" in sys.argv
CALLS = 20000


def timed(f, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters                     # microseconds per call


lines = [f"Actuation stage, {torch.cuda.get_device_name(0)}",
         "microseconds per env step, back-to-back launches on one stream (host enqueue included: the stage is launch-latency bound);",
         f"five alternated windows of {CALLS} calls (0.2 - 0.7 s each): min / median / max.  Fresh output tensors per call in every form, as in the env.",
         ""]
for n, d in ((4096, 69),) if TRACE else ((4096, 69), (4096, 153), (16384, 69)):
    act = (1.5 * torch.randn(n, d, generator=g)).to(dev)
    ref, sim = (0.3 * torch.randn(n, d, generator=g)).to(dev), (0.3 * torch.randn(n, d, generator=g)).to(dev)
    offset, scale = torch.zeros(d, device=dev), (0.3 + 3.0 * torch.rand(d, generator=g)).to(dev)
    freeze = torch.zeros(d, dtype=torch.uint8, device=dev)
    freeze[9:12] = 1

    def eager_plain():
        a = torch.clamp(act, -1.0, 1.0)
        return a, torch.addcmul(offset, scale, a)

    def eager_res():
        a = torch.clamp(act, -1.0, 1.0)
        t = ref + scale * a
        return a, torch.maximum(torch.minimum(t, sim + math.pi / 2), sim - math.pi / 2)

    calls = {
        "pulse_pd_targets (plain)": lambda: ops.pd_targets(act, scale, clip=1.0, offset=offset),
        "torch.clamp + torch.addcmul (the two launches before)": eager_plain,
        "pulse_pd_targets (plain, freeze mask)": lambda: ops.pd_targets(act, scale, clip=1.0, offset=offset, freeze=freeze),
        "pulse_pd_targets (res_action)": lambda: ops.pd_targets(act, scale, clip=1.0, ref_dof_pos=ref, sim_dof_pos=sim),
        "torch.clamp + res_action chain (7 launches before)": eager_res,
    }
    for f in calls.values():
        for _ in range(200):
            f()
    if TRACE:
        torch.cuda.synchronize()
        sys.exit(0)
    res = {k: [] for k in calls}
    for rep in range(5):
        for k, f in calls.items():
            res[k].append(timed(f, CALLS))
    same = all(torch.equal(x.nan_to_num(), y.nan_to_num()) for x, y in zip(calls["pulse_pd_targets (plain)"](), eager_plain())) and \
        all(torch.equal(x.nan_to_num(), y.nan_to_num()) for x, y in zip(calls["pulse_pd_targets (res_action)"](), eager_res()))
    lines.append(f"N = {n}, D = {d}   (outputs equal to the eager forms: {same})")
    for k, v in res.items():
        v = sorted(v)
        lines.append(f"  {k:56s} {v[0]:7.2f} {v[2]:7.2f} {v[-1]:7.2f}")
    lines.append("")
text = "\n".join(lines)
print(text)
if len(sys.argv) > 1 and not TRACE:
    with open(sys.argv[1], "w") as fh:
        fh.write(text)
