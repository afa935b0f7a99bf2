"""Plain-torch restatement of PHC's MCP composer stage (TEST INFRASTRUCTURE -- never imported by pulse_amd).

  * ``McpTwin``: AMPMCPBuilder.Network (phc/learning/amp_network_mcp_builder.py:23-87) as nn.Modules carrying the reference's parameter names
    in its creation order -- AMPBuilder.Network's actor_mlp, critic_mlp, value, mu, sigma (network_builder.py:245-261), then the composer
    ``_build_mlp(units + [num_prim], activation)`` with every layer activated (:41-51) and an nn.Softmax(dim=1) behind it when has_softmax
    (:53-55).  ``eval_actor`` is :64-86 (mu = the composer's output, sigma = mu * 0 + sigma), ``eval_critic`` the plain critic + value head.
    ``a2c_network`` also carries the attributes the reference's own eval_actor body reads, so that body runs on the twin's modules.
  * ``pnn_columns`` / ``compose``: HumanoidImMCP.step's composition (phc/env/tasks/humanoid_im_mcp.py:51-67) over a load_pnn-shaped state dict
    (PNN forward phc/learning/pnn.py:84-131, like oracle.agent_oracle.oracle_pnn_teacher_action).
"""
import torch
from torch import nn

ACTS = {"relu": nn.ReLU, "silu": nn.SiLU}


def _mlp(in_dim, units, act):
    layers = []
    for u in units:
        layers += [nn.Linear(in_dim, u), act()]
        in_dim = u
    return nn.Sequential(*layers)


class _A2CNetwork(nn.Module):
    def __init__(self, obs_size, units, num_prim, activation, has_softmax, sigma_val):
        super().__init__()
        act = ACTS[activation]
        self.actor_cnn = nn.Sequential()                               # "This is empty" (:66)
        self.actor_mlp = _mlp(obs_size, units, act)                    # created, saved, never evaluated (:64-86)
        self.critic_mlp = _mlp(obs_size, units, act)
        self.value = nn.Linear(units[-1], 1)
        self.mu = nn.Linear(units[-1], num_prim)                       # created, saved, never evaluated
        self.sigma = nn.Parameter(torch.full((num_prim,), float(sigma_val)), requires_grad=False)
        self.composer = _mlp(obs_size, list(units) + [num_prim], act)
        if has_softmax:
            self.composer.append(nn.Softmax(dim=1))
        for m in self.modules():                                       # network_builder.py:273-277: biases zeroed
            if isinstance(m, nn.Linear):
                nn.init.zeros_(m.bias)
        self.is_discrete, self.is_multi_discrete, self.is_continuous = False, False, True
        self.space_config = {"fixed_sigma": True}
        self.sigma_act = nn.Identity()


class McpTwin(nn.Module):
    def __init__(self, obs_size, units, num_prim, activation="relu", has_softmax=True, sigma_val=-2.9):
        super().__init__()
        self.a2c_network = _A2CNetwork(obs_size, list(units), num_prim, activation, has_softmax, sigma_val)

    def eval_actor(self, obs):
        net = self.a2c_network
        mu = net.composer(net.actor_cnn(obs).contiguous().view(obs.size(0), -1))
        return mu, mu * 0.0 + net.sigma_act(net.sigma)

    def eval_critic(self, obs):
        net = self.a2c_network
        return net.value(net.critic_mlp(obs))

    def layout(self):
        """[(name, shape)] of the trainable tensors in creation order (sigma, a fixed buffer of the checkpoint, left out)."""
        return [(k, tuple(v.shape)) for k, v in self.named_parameters() if not k.endswith(".sigma")]

    def state_dict_ref(self):
        return {k: v.detach().clone() for k, v in self.state_dict().items()}


def pnn_columns(pnn_model, num_prim, activation, full_obs, has_lateral=False):
    """PNN.forward's per-column actions stacked on dim 1 (pnn.py:84-131): (N, num_prim, A)."""
    act = ACTS[activation]

    def seq(prefix):
        layers, i = [], 0
        while f"{prefix}.{2 * i}.weight" in pnn_model:
            w, b = pnn_model[f"{prefix}.{2 * i}.weight"], pnn_model[f"{prefix}.{2 * i}.bias"]
            lin = nn.Linear(w.shape[1], w.shape[0])
            with torch.no_grad():
                lin.weight.copy_(w)
                lin.bias.copy_(b)
            layers += [lin, act()]
            i += 1
        return nn.Sequential(*layers[:-1])

    with torch.no_grad():
        if not has_lateral:
            return torch.stack([seq(f"a2c_network.pnn.actors.{k}")(full_obs) for k in range(num_prim)], dim=1)
        cols, h1s = [], []
        for c in range(num_prim):
            net = seq(f"a2c_network.pnn.actors.{c}")
            h1 = net[:2](full_obs)
            lat = [torch.nn.functional.linear(h1s[j], pnn_model[f"a2c_network.pnn.u.{c - 1}.{j}.0.weight"]) for j in range(len(h1s))]
            cols.append(net[4](net[3](net[2](h1) + sum(lat))))
            h1s.append(h1)
        return torch.stack(cols, dim=1)


def normalize_obs(obs, running_mean, running_var):
    """humanoid_im_mcp.py:53-55."""
    return torch.clamp((obs - running_mean.float()) / torch.sqrt(running_var.float() + 1e-05), min=-5.0, max=5.0)


def mix(weights, x_all, discrete=False):
    """humanoid_im_mcp.py:56-58, 67."""
    if discrete:
        weights = torch.nn.functional.one_hot(torch.argmax(weights, dim=1), num_classes=x_all.shape[1]).float()
    return torch.sum(weights[:, :, None] * x_all, dim=1)


def compose(checkpoint, num_prim, activation, obs, weights, discrete=False, has_lateral=False):
    """HumanoidImMCP.step's composition (:51-67) on an observation buffer: the (N, A) joint targets handed to pre_physics_step."""
    rms = checkpoint["running_mean_std"]
    with torch.no_grad():
        full_obs = normalize_obs(obs, rms["running_mean"], rms["running_var"])
        return mix(weights, pnn_columns(checkpoint["model"], num_prim, activation, full_obs, has_lateral), discrete)
