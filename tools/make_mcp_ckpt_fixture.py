"""GPU-side generator of tests/golden/ckpt_mcp_small.pt (run on the MI355X box; uses pulse_amd only):

    python tools/make_mcp_ckpt_fixture.py out/ckpt_mcp_small.pt

A small amp_mcp agent (``mcp_small``, has_softmax: False, units [96, 64]) is trained for two epochs.  The file keeps the composer's tensors of
its checkpoint (the keys the reference's load_mcp_mlp(..., mlp_name="composer") reads, phc/learning/network_loader.py:11-52), the names and
shapes of EVERY tensor of the checkpoint's 'model', the observation statistics, a few raw observations and the mu the HIP path computed from
them.  tests/test_mcp_cpu.py feeds it to the reference's loader and compares mu."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pulse_amd import configs

out = sys.argv[1]
dev = "cuda:0"
net = dict(configs.NETWORK_MCP, mlp=dict(configs.NETWORK_MCP["mlp"], units=[96, 64]))
agent, _ = configs.make_agent("mcp_small", device=dev, seed=77, network=net)
for e in range(2):
    agent.epoch_num = e + 1
    agent.train_epoch()
ck = agent.get_full_state_weights()
n = 24
obs = agent.vec_env.task.obs_buf
ws = agent.model.workspace(obs.shape[0], train=False)
agent.set_eval()
agent._preproc_obs(obs, ws, obs.shape[0])
agent.model.forward(ws, obs.shape[0])
cpu = lambda v: v.detach().cpu().clone()
fx = {"model": {k: cpu(v) for k, v in ck["model"].items() if k.startswith("a2c_network.composer.")},
      "model_layout": [(k, tuple(v.shape)) for k, v in ck["model"].items()],
      "running_mean_std": {k: cpu(v) for k, v in ck["running_mean_std"].items()},
      "fixture": {"obs_buf": cpu(obs[:n]), "mu": cpu(ws["mu"][:n]), "network": net}}
torch.save(fx, out)
print("saved", out, os.path.getsize(out), "bytes")
print(fx["model_layout"])
