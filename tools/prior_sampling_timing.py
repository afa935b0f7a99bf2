"""One launch set of the cfg3 policy step, many times and nothing else: the run to put under
`rocprofv3 --kernel-trace --stats` for profiles/prior_sampling.txt (summarised by tools/rocprof_summary.py).

    python tools/prior_sampling_timing.py --set posterior    encoder plan + pulse_vae_embed + decoder plan   (what a tracking step costs)
    python tools/prior_sampling_timing.py --set prior        prior plan + pulse_vae_embed_prior + decoder plan   (a generation step)
    python tools/prior_sampling_timing.py --set kernels      the two head launches alone, on the same rows

[--rows 8192] [--iters 100] [--root DIR]: ``--root`` imports pulse_amd from another checkout (the parent commit, for its posterior step; it
has no 'prior' set).  The network is cfg3's (configs.NETWORK_Z, 934-column observation, 32 latents) with its initial weights; fresh noise
is drawn per step, as in the product path.  Prints the step's wall time per iteration as well (host enqueue included).
"""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--set", choices=("posterior", "prior", "kernels"), required=True)
ap.add_argument("--rows", type=int, default=8192)
ap.add_argument("--iters", type=int, default=100)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, args.root)

import torch  # noqa: E402

from pulse_amd import configs  # noqa: E402
from pulse_amd import kernels as K  # noqa: E402
from pulse_amd.learning.model_z import AMPZModel  # noqa: E402

dev = torch.device("cuda:0")
torch.manual_seed(0)
m, E, S = args.rows, 32, 358
detail = {k: configs.ENV_IM_VAE[k] for k in ("embedding_size", "embedding_norm", "z_type", "use_vae_prior", "use_vae_clamped_prior", "vae_var_clamp_max")}
model = AMPZModel(configs.NETWORK_Z, actions_num=69, self_obs_size=S, task_obs_size=576, task_obs_size_detail=detail, device=dev,
                  generator=torch.Generator(device=dev).manual_seed(0)).eval()
ws = model.workspace(m, train=False)
ws["x"].zero_()
ws["x"][:, :934] = torch.randn(m, 934, device=dev).clamp(-5, 5)

if args.set == "kernels":
    bufs, zc = ws["g"].act_bufs, model.net.z_col
    zh, ph = torch.randn(m, 2 * E, device=dev), torch.randn(m, 2 * E, device=dev)
    eps = torch.randn(m, E, device=dev)

    def step():
        K.vae_embed(zh, ws["x"], bufs["ain"], rows=m, embedding_size=E, self_obs_size=S, z_col=zc, eps=eps, cin=bufs["cin"], clamp=True, clamp_max=2.0)
        K.vae_embed_prior(ph, ws["x"], bufs["ain"], rows=m, embedding_size=E, self_obs_size=S, z_col=zc, eps=eps, cin=bufs["cin"], clamp=True, clamp_max=2.0)
else:
    if args.set == "prior":
        model.z_source = "prior"

    def step():
        model.forward_actor(ws, m)

for _ in range(3):
    step()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(args.iters):
    step()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print(f"[{args.set}] root {args.root}: {args.rows} rows, {args.iters} + 3 steps, {1e6 * dt / args.iters:.1f} us per step (wall, host enqueue included)")
