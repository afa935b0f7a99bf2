"""The terrain-task policy network (``network: amp_sept``) on the gfx950 kernels.

Mirrors AMPSeptBuilder.Network, phc/learning/amp_network_sept_builder.py:19-165 (registered at run_hydra.py:260; config
phc/data/cfg/learning/pulse_z_terrain.yaml:12-44): the observation is [self obs | task obs], the task part (trajectory samples + height
map, 1044 floats) goes through a task MLP ([512, 256] SiLU, both layers activated) and the actor / critic MLPs ([2048, 1024, 512] SiLU)
read cat(self_obs, task_out) (358 + 256).

One reference quirk is structural and mirrored: with ``separate: True`` the constructor calls ``_build_task_mlp()`` twice
(:33-36) and both calls assign ``self._task_mlp`` -- so there is ONE task MLP, shared by eval_actor (:92-101) and eval_critic
(:77-90), and its weights receive the sum of both gradients.  (The first instance is garbage-collected; only its RNG draws remain.)
The crowd variant of the terrain task (env/humanoid_tasks.py: divide_group / group_obs / velocity_map) is built, this network's side of it
is not -- and cannot follow the reference: eval_task (:48-60) feeds the slice [traj | people] to ``_task_mlp``, which was built for
traj + heightmap inputs (:107-111), so the 'people' branch fails in the first matmul, and ``_build_task_mlp`` asserts 'heightmap' in the
detail (:107), which a velocity_map observation ('heightmap_velocity') does not carry.  Both raise here, saying so; the flat networks
(amp, amp_z_reader) read the wider observation as it is.  People stamped into the height map without velocity_map leave the widths alone
and train on this network unchanged.

Physical layout (learning/graph.py): the task MLP reads the observation buffer from column 356 (16-byte aligned; the two self-observation
columns in front carry zero weights through the layer's column map), its last layer writes straight into columns 360..615 of the actor's
concat buffer, a copy places the same 256 values (and the self observation) in the critic's; backward runs actor and critic down to
their concat buffers (SiLU derivative of the task output fused into both input-gradient GEMMs), adds the two task-output gradients and
continues through the task MLP.
"""
from .. import kernels as K
from .graph import GraphModel, GraphNetwork, Linear, r4


class AMPSeptNetwork(GraphNetwork):
    def __init__(self, params, *, actions_num, self_obs_size, task_obs_size, task_obs_size_detail, device="cuda:0", split_k=8):
        d = dict(task_obs_size_detail or {})
        if "people" in d:
            raise NotImplementedError("amp_sept with a 'people' block (divide_group + group_obs) is not built: the reference's eval_task "
                                      "(phc/learning/amp_network_sept_builder.py:48-60) feeds a [traj | people] slice to the task MLP, which was built "
                                      "for traj + heightmap inputs (:107-111), so it cannot run either; use a flat network (amp, amp_z_reader), which "
                                      "reads the wider observation as it is")
        if "heightmap_velocity" in d:
            raise ValueError("amp_sept needs 'heightmap' in task_obs_size_detail, got 'heightmap_velocity' (velocity_map): the reference asserts "
                             "'heightmap' when it builds the task MLP (phc/learning/amp_network_sept_builder.py:107) and cannot run with "
                             "velocity_map either; use a flat network (amp, amp_z_reader)")
        if "traj" not in d or "heightmap" not in d:
            raise ValueError("amp_sept needs task_obs_size_detail with 'traj' and 'heightmap' (amp_network_sept_builder.py:107)")
        if d["traj"] + d["heightmap"] != task_obs_size:
            raise ValueError("task_obs_size_detail does not add up to task_obs_size")
        self.units = [int(u) for u in params["mlp"]["units"]]
        self.task_units = [int(u) for u in params["task_mlp"]["units"]]
        self.act = K.ACTIVATIONS[params["mlp"]["activation"]]
        self.task_act = K.ACTIVATIONS[params["task_mlp"]["activation"]]
        S, TU = int(self_obs_size), self.task_units[-1]
        self.t_col = r4(S)                                       # 360: where the task embedding starts inside cat(self_obs, task_out)
        self.cat_width = self.t_col + TU
        self.cat_map = list(range(S)) + list(range(self.t_col, self.t_col + TU))
        self.task_src_col = S // 4 * 4                           # 356: aligned start of the task MLP's input window
        self.task_map = list(range(S - self.task_src_col, S - self.task_src_col + int(task_obs_size)))
        super().__init__(params, actions_num=actions_num, self_obs_size=self_obs_size, task_obs_size=task_obs_size, device=device, split_k=split_k)

    def _build(self, m, x=None):
        S, U, T = self.self_obs_size, self.units, self.task_units
        g, book = self._new_graph(m, x), self.book
        g.buffer("ain", self.cat_width)
        g.buffer("cin", self.cat_width)
        lins = {}
        names_a, names_c = ["a1", "a2", "a3", "a4"][:len(U)], ["c1", "c2", "c3", "c4"][:len(U)]
        # the task output sits in columns t_col.. of BOTH concat buffers; its pre-activation is kept beside the actor's copy
        tc = (self.t_col, self.cat_width, self.task_act, "ain", 0)
        # A2CBuilder order: actor_mlp, critic_mlp, value, mu (network_builder.py:245-261), then the task MLP (amp_network_sept_builder.py:33-36)
        lins["actor_mlp"] = g.mlp("a2c_network.actor_mlp", "ain", S + T[-1], U, self.act, names_a, colmap=self.cat_map, first_grad_ranges=[tc], tag="actor")
        lins["critic_mlp"] = g.mlp("a2c_network.critic_mlp", "cin", S + T[-1], U, self.act, names_c, colmap=self.cat_map, first_grad_ranges=[tc],
                                   tag="critic")
        g.buffer("value", 1)
        g.buffer("mu", self.actions_num)
        lins["value"] = g.linear(Linear(book, "a2c_network.value", U[-1], 1), names_c[-1], "value", grad_ranges=[(0, U[-1], self.act, names_c[-1], 0)], tag="critic")
        lins["mu"] = g.linear(Linear(book, "a2c_network.mu", U[-1], self.actions_num), names_a[-1], "mu", grad_ranges=[(0, U[-1], self.act, names_a[-1], 0)], tag="actor")
        # _task_mlp = Sequential(Linear, SiLU, Linear, SiLU): every layer activated; the last one writes the actor's concat slot
        task = []
        cur, cur_w = "x", self.task_obs_size
        for i, u in enumerate(T):
            last = i == len(T) - 1
            lin = Linear(book, f"a2c_network._task_mlp.{2 * i}", cur_w, u, self.task_act, self.task_map if i == 0 else None)
            dst = "ain" if last else f"t{i + 1}"
            if not last:
                g.buffer(dst, u)
            gr = None if i == 0 else [(0, cur_w, self.task_act, cur, 0)]
            g.linear(lin, cur, dst, src_col=self.task_src_col if i == 0 else 0, dst_col=self.t_col if last else 0, grad_ranges=gr, tag="task")
            task.append(lin)
            cur, cur_w = dst, u
        lins["task_mlp"] = task
        return {"graph": g, "lins": lins}

    def _plans(self, g):
        return {"fwd_task": g.forward_plan({"task"}), "fwd_actor": g.forward_plan({"actor"}), "fwd_critic": g.forward_plan({"critic"}),
                "bwd_actor": g.backward_plan({"actor"}), "bwd_critic": g.backward_plan({"critic"}), "bwd_task": g.backward_plan({"task"})}


class AMPSeptModel(GraphModel):
    """The model interface CommonAgent / AMPAgent drive (workspace / forward / eval_critic / backward over one flat buffer)."""
    network = AMPSeptNetwork
    mixed_precision = False

    def _task(self, ws, critic_only=False):
        """eval_task (:43-60) once, then cat([self_obs, task_out]) for both consumers (:84-86, 96-98)."""
        net, g = self.net, ws["g"]
        S, tc, cw = net.self_obs_size, net.t_col, net.cat_width
        ws["G"]["fwd_task"].run()
        ain, cin = g.act_bufs["ain"], g.act_bufs["cin"]
        ain[:, :S].copy_(ws["x"][:, :S])
        cin[:, :S].copy_(ws["x"][:, :S])
        cin[:, tc:cw].copy_(ain[:, tc:cw])

    def forward(self, ws, m):
        self._task(ws)
        ws["G"]["fwd_actor"].run()
        ws["G"]["fwd_critic"].run()

    def eval_critic(self, ws, m):
        self._task(ws)
        ws["G"]["fwd_critic"].run()

    def backward(self, ws, m, grad_scale=1.0, sq_partials=None, on_bucket=None):
        """d loss / d (mu, value) are in ws['dmu'] / ws['dval'].  The shared task MLP receives the sum of the actor's and the critic's
        gradient at its output (both already carry the SiLU derivative from the fused input-gradient epilogues).  Every layer is visited,
        so the region reduce reads exactly the slabs the weight-gradient launches wrote (no zero fill of the slab buffer) and leaves the norm
        clip's sums of squares in ``sq_partials``."""
        net, g = self.net, ws["g"]
        tc, cw = net.t_col, net.cat_width
        ws["G"]["bwd_actor"].run()
        ws["G"]["bwd_critic"].run()
        g.grad("ain")[:, tc:cw].add_(g.grad("cin")[:, tc:cw])
        ws["G"]["bwd_task"].run()
        return self._reduce(grad_scale, self._untouched(ws, ("actor", "critic", "task")), sq_partials)
