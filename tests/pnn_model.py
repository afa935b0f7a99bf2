"""Plain-torch restatement of PHC's primitive stage (TEST INFRASTRUCTURE -- never imported by pulse_amd).

  * ``PnnColumns``: PNN (phc/learning/pnn.py:13-131) as nn.Modules under the reference's parameter names in its creation order: ``actors``
    (one ``Sequential(Linear, act, ..., Linear(units[-1], actions))`` per column), with ``has_lateral`` the bias-free links ``u[i][j]`` =
    ``Sequential(Linear(units[0], units[1]), .., Linear(units[-1], actions))`` (:27-39); ``freeze_pnn`` is :41-46 (slices and all),
    ``forward(x, idx)`` is :84-131.
  * ``PnnTwin``: AMPPNNBuilder.Network (phc/learning/amp_network_pnn_builder.py:25-89): AMPBuilder.Network's actor_mlp, critic_mlp, value, mu,
    sigma (network_builder.py:245-267), ``del actor_mlp`` (:52), then ``pnn`` and ``freeze_pnn(training_prim)``.  ``eval_actor`` is :62-89
    (mu = pnn(obs, idx=training_prim)[0], sigma = mu * 0 + sigma), ``eval_critic`` the plain critic + value head.  ``a2c_network`` also carries
    the attributes the reference's own eval_actor body reads, so that body runs on the twin's modules.
  Biases are zeroed, the columns' too (pulse_amd/learning/network_pnn.py draws the same way, so a shared seed gives the same network).
"""
from collections import defaultdict

import torch
from torch import nn

ACTS = {"relu": nn.ReLU, "silu": nn.SiLU}


def _mlp(in_dim, units, act, out=None):
    layers = []
    for u in units:
        layers += [nn.Linear(in_dim, u), act()]
        in_dim = u
    if out is not None:
        layers.append(nn.Linear(in_dim, out))
    return nn.Sequential(*layers)


class PnnColumns(nn.Module):
    def __init__(self, in_dim, units, output_size, num_cols, has_lateral, activation):
        super().__init__()
        act = ACTS[activation]
        self.numCols, self.has_lateral = num_cols, has_lateral
        self.actors = nn.ModuleList([_mlp(in_dim, units, act, output_size) for _ in range(num_cols)])
        if has_lateral:
            self.u = nn.ModuleList()
            for i in range(num_cols - 1):
                self.u.append(nn.ModuleList())
                for _ in range(i + 1):
                    u, k = nn.Sequential(), units[0]
                    for unit in units[1:]:
                        u.append(nn.Linear(k, unit, bias=False))
                        k = unit
                    u.append(nn.Linear(units[-1], output_size, bias=False))
                    self.u[i].append(u)

    def freeze_pnn(self, idx):
        for p in self.actors[:idx].parameters():
            p.requires_grad = False
        if self.has_lateral:
            for p in self.u[:idx - 1].parameters():
                p.requires_grad = False

    def forward(self, x, idx=-1):
        if not self.has_lateral:
            if idx != -1:
                a = self.actors[idx](x)
                return a, [a]
            acts = [self.actors[i](x) for i in range(self.numCols)]
            return acts, acts
        if idx == 0:
            a = self.actors[0](x)
            return a, [a]
        if idx == -1:
            idx = self.numCols - 1
        cache = defaultdict(list)
        for c in range(idx + 1):
            col = self.actors[c]
            assert len(col) == 5
            h1 = col[:2](x)
            lat = [self.u[c - 1][j][0](cache[0][j]) for j in range(len(cache[0]))]
            h2 = col[3](col[2](h1) + sum(lat))
            a = col[4](h2)
            cache[0].append(h1)
            cache[1].append(h2)
            cache[2].append(a)
        return a, cache[2]


class _A2CNetwork(nn.Module):
    def __init__(self, obs_size, units, actions_num, num_prim, training_prim, has_lateral, activation, sigma_val):
        super().__init__()
        act = ACTS[activation]
        self.actor_cnn = nn.Sequential()                                # "This is empty" (:65)
        self.actor_mlp = _mlp(obs_size, units, act)
        self.critic_mlp = _mlp(obs_size, units, act)
        self.value = nn.Linear(units[-1], 1)
        self.mu = nn.Linear(units[-1], actions_num)                     # created, saved, never evaluated (:81-82)
        self.sigma = nn.Parameter(torch.full((actions_num,), float(sigma_val)), requires_grad=False)
        del self.actor_mlp                                              # :52
        self.pnn = PnnColumns(obs_size, units, actions_num, num_prim, has_lateral, activation)
        for m in self.modules():
            if isinstance(m, nn.Linear) and m.bias is not None:
                nn.init.zeros_(m.bias)
        self.pnn.freeze_pnn(training_prim)
        self.training_prim = training_prim
        self.is_discrete, self.is_multi_discrete, self.is_continuous = False, False, True
        self.space_config = {"fixed_sigma": True}
        self.sigma_act = nn.Identity()


class PnnTwin(nn.Module):
    def __init__(self, obs_size, units, actions_num, num_prim, training_prim, has_lateral=False, activation="relu", sigma_val=-2.9):
        super().__init__()
        self.a2c_network = _A2CNetwork(obs_size, list(units), actions_num, num_prim, training_prim, has_lateral, activation, sigma_val)

    def eval_actor(self, obs):
        net = self.a2c_network
        mu = net.pnn(net.actor_cnn(obs).contiguous().view(obs.size(0), -1), idx=net.training_prim)[0]
        return mu, mu * 0.0 + net.sigma_act(net.sigma)

    def eval_critic(self, obs):
        net = self.a2c_network
        return net.value(net.critic_mlp(obs))

    def columns(self, obs):
        """Every column's action, (N, num_prim, A): PNN.forward(x, idx=-1)[1]."""
        return torch.stack(list(self.a2c_network.pnn(obs, idx=-1)[1]), dim=1)

    def layout(self):
        """[(name, shape)] of the tensors in creation order (sigma, a fixed buffer of the checkpoint, left out)."""
        return [(k, tuple(v.shape)) for k, v in self.named_parameters() if not k.endswith(".sigma")]

    def state_dict_ref(self):
        return {k: v.detach().clone() for k, v in self.state_dict().items()}

    def jitter_biases(self, scale=0.1):
        """Biases are zero-initialised: move them off zero so a dropped bias shows."""
        with torch.no_grad():
            for k, p in self.named_parameters():
                if p.dim() == 1 and not k.endswith(".sigma"):
                    p.add_(scale * torch.randn_like(p))
        return self
