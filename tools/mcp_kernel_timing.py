"""GPU: one timing of the three MCP kernels (csrc/mcp.hip) at N = 4096, P = 4, A = 69, the compose kernel beside the torch expression
learning/teacher.py uses for the same mixture, alternated in one process.  A record (profiles/mcp_kernels.txt), not a gate.

    python tools/mcp_kernel_timing.py [out.txt]
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pulse_amd import kernels as K, ops
from pulse_amd._lib import ACT_RELU

dev = "cuda:0"
N, P, A, AP = 4096, 4, 69, 72
g = torch.Generator().manual_seed(0)
w = torch.rand(N, P, generator=g).to(dev)
x = torch.randn(N, P, AP, generator=g).to(dev)
out_k, out_t = torch.zeros(N, A, device=dev), torch.zeros(N, A, device=dev)
h, mu, dmu, dz = w.clone(), torch.zeros(N, P, device=dev), torch.randn(N, P, device=dev), torch.zeros(N, P, device=dev)
xs = x[:, :, :A]

calls = {
    "pulse_mcp_compose": lambda: ops.mcp_compose(w, x, out_k, num_actions=A),
    "torch.sum(w[:, :, None] * x, dim=1, out=)": lambda: torch.sum(w[:, :, None] * xs, dim=1, out=out_t),
    "pulse_mcp_head_forward": lambda: K.mcp_head_forward(h, mu, rows=N, num_prim=P),
    "pulse_mcp_head_backward (softmax + relu)": lambda: K.mcp_head_backward(dmu, dz, rows=N, num_prim=P, mu=mu, aux=h, activation=ACT_RELU),
}


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
for rep in range(5):                                              # alternated: five windows of 2000 back-to-back calls each
    for k, f in calls.items():
        res[k].append(timed(f, 2000))
diff = (out_k - out_t).abs().max().item()
lines = [f"MCP kernels, N = {N}, P = {P}, A = {A} (a_pitch {AP}), {torch.cuda.get_device_name(0)}",
         "microseconds per call, back-to-back launches on one stream (host enqueue included: these kernels are launch-latency bound);",
         "five alternated windows of 2000 calls: min / median / max",
         ""]
for k, v in res.items():
    v = sorted(v)
    lines.append(f"{k:48s} {v[0]:7.2f} {v[2]:7.2f} {v[-1]:7.2f}")
lines += ["", f"max |pulse_mcp_compose - torch| = {diff:.3e}"]
text = "\n".join(lines) + "\n"
print(text)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write(text)
