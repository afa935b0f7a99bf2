"""CPU: the batch bookkeeping of the evaluation sweep (pulse_amd/learning/eval_sweep.py) against the reference's own method body,
IMAmpAgent._post_step_eval (phc/learning/im_amp.py:244-363), run on stubs: 7 unique motions on 3 envs -- three batches, the last one
wrapping around the data set -- under scripted ``terminate`` sequences.  The reference side is extracted by name through oracle/refload
and recorded with RefRecord (tests/golden/ref/), so the test replays where the reference checkout is absent.  Also: the evaluation body
list against Humanoid._eval_bodies (humanoid.py:381-388)."""
import ast
import os
import types

import numpy as np
import pytest
import torch

from oracle import refload
from oracle.refrecord import RefRecord
from pulse_amd import synthetic as syn
from pulse_amd.env.humanoid_im import eval_body_names
from pulse_amd.learning.eval_sweep import EvalSweep

N, U = 3, 7
NUM_STEPS = [6, 5, 4, 5, 3, 4, 3]                  # get_motion_num_steps of the 7 clips
KEYS = [f"clip_{i}" for i in range(U)]

# terminate flags per batch: {batch step (0-based, the value of curr_steps when the step is judged): envs that report terminate}
SCRIPTS = {
    # batch 0 (clips 0 1 2): env 1 fails at step 2; env 2 (4 steps) reports a termination at step 4, one step after its last frame: no failure
    # batch 1 (clips 3 4 5): every env terminates early -> the batch ends there
    # batch 2 (clips 6 0 1, wrapped): only env 0 is inside the bound; env 2's failure is cut off with the wrapped tail
    "mixed": [{2: [1], 4: [2]}, {1: [0, 1], 2: [2]}, {1: [2]}],
    # the last clip itself fails in the wrapped batch while the envs behind the bound live on: curr_max = curr_steps - 1, the batch ends at once
    "last_clip_fails": [{}, {2: [1]}, {1: [0]}],
    # nothing fails; a termination exactly AT a clip's last counted step (curr_steps == num_steps - 1) does count
    "edge_counts": [{3: [2]}, {}, {}],
}


def _resident(start_idx):
    ids = (torch.arange(N) + start_idx) % U
    return ids, torch.tensor([NUM_STEPS[i] for i in ids.tolist()], dtype=torch.int32)


def _terminate(script, batch, step):
    t = torch.zeros(N, dtype=torch.bool)
    t[script[batch].get(step, [])] = True
    return t


def _run_reference(script):
    """The reference's _post_step_eval on stubs; returns batch lengths, terminate history, success rate, failed / success keys."""
    path = os.path.join(refload.REFERENCE_ROOT, "phc", "learning", "im_amp.py")
    ns = refload._namespace()
    five = ("mpjpe_g", "mpjpe_l", "mpjpe_pa", "accel_dist", "vel_dist")
    ns["compute_metrics_lite"] = lambda pred, gt: {k: np.zeros(1) for k in five} if len(pred) else {}
    ns["print"] = lambda *a, **k: None
    exec(compile(refload._extract(path, ["_post_step_eval"], methods_of="IMAmpAgent")["_post_step_eval"], "<reference:IMAmpAgent._post_step_eval>", "exec"), ns)
    lib = types.SimpleNamespace(_num_unique_motions=U, _motion_data_keys=np.array(KEYS))
    env = types.SimpleNamespace(num_envs=N, start_idx=0, _motion_lib=lib)

    def load():
        lib._curr_motion_ids, steps = _resident(env.start_idx)
        lib.get_motion_num_steps = lambda: steps

    def forward():
        env.start_idx += N
        load()
    env.forward_motion_samples = forward
    load()
    pbar = types.SimpleNamespace(clear=lambda: None, update=lambda n: None, refresh=lambda: None, set_description=lambda s: None)
    agent = types.SimpleNamespace(curr_stpes=0, terminate_state=torch.zeros(N), terminate_memory=[], mpjpe=[], mpjpe_all=[], gt_pos=[], gt_pos_all=[],
                                  pred_pos=[], pred_pos_all=[], success_rate=0, pbar=pbar, device="cpu", vec_env=types.SimpleNamespace(env=types.SimpleNamespace(task=env)))
    lengths, batch, step = [], 0, 0
    with np.errstate(all="ignore"):
        while True:
            info = {"terminate": _terminate(script, batch, step), "mpjpe": torch.zeros(N), "body_pos": np.zeros((N, 2, 3)), "body_pos_gt": np.zeros((N, 2, 3))}
            done, out = ns["_post_step_eval"](agent, info, torch.zeros(N))
            step += 1
            if out["end"] or bool(done.all()):
                lengths.append(step)
                batch, step = batch + 1, 0
            if out["end"]:
                break
    hist = np.concatenate(agent.terminate_memory)
    return {"lengths": lengths, "memory": torch.as_tensor(hist.astype(np.uint8)), "success_rate": float(agent.success_rate),
            "failed": [str(k) for k in out["failed_keys"]], "success": [str(k) for k in out["success_keys"]]}


def _run_sweep(script, max_steps=None):
    sweep = EvalSweep(N, U, max_steps=max_steps)
    start_idx, batch, step = 0, 0, 0
    while True:
        ids, steps = _resident(start_idx)
        batch_end, end = sweep.post_step(_terminate(script, batch, step).to(torch.int64), steps, ids, start_idx)
        step += 1
        if batch_end:
            sweep.end_batch(torch.zeros(N, 8, dtype=torch.float64))
            batch, step, start_idx = batch + 1, 0, start_idx + N
        if end:
            return sweep


@pytest.mark.parametrize("name", sorted(SCRIPTS))
def test_sweep_is_the_reference_post_step_eval(request, name):
    script = SCRIPTS[name]
    with RefRecord(request) as R:
        ref = _run_reference(script) if R.live else None
        lengths = R.obj("batch_lengths", lambda: ref["lengths"])
        memory = R.t("terminate_memory", lambda: ref["memory"])
        rate = R.obj("success_rate", lambda: ref["success_rate"])
        failed = R.obj("failed_keys", lambda: ref["failed"])
        success = R.obj("success_keys", lambda: ref["success"])
        sweep = _run_sweep(script)
        assert sweep.batch_lengths == lengths
        assert torch.equal(torch.cat(sweep.terminate_memory).to(torch.uint8), memory)
        assert sweep.success_rate == rate
        got_failed, got_success = sweep.keys(KEYS)
        assert got_failed == failed and got_success == success
        assert len(memory) == 3 * N and len(failed) + len(success) == U          # three batches; the wrapped tail is cut off
    # what the scripts are there for, stated independently of the recording
    if name == "mixed":
        assert lengths == [6, 3, 3] and failed == ["clip_1", "clip_3", "clip_4", "clip_5"]
        assert memory.tolist() == [0, 1, 0, 1, 1, 1, 0, 0, 1]                   # env 2 of batch 0: terminated after its last frame, not a failure
    elif name == "last_clip_fails":
        assert lengths == [6, 5, 2] and failed == ["clip_4", "clip_6"]
    else:
        assert failed == ["clip_2"] and lengths[0] == 6


def test_max_steps_caps_a_batch_and_means_are_frame_weighted():
    sweep = _run_sweep([{}, {}, {}], max_steps=2)
    assert sweep.batch_lengths == [2, 2, 2] and sweep.keys(KEYS)[0] == []
    # motion i: 2 (i + 1) frames with a per-frame error of (i + 1) mm (i + 1 velocity frames of 3 (i + 1) mm); rows 7, 8 are the wrapped tail
    rows = torch.tensor([[2.0 * k * k, 0.0, 0.0, 3.0 * k * k, 0.0, 2.0 * k, 1.0 * k, 1.0] for k in range(1, 3 * N + 1)], dtype=torch.float64)
    sweep.accum_memory = list(rows.split(N))
    sweep.terminate_memory[1][0] = True                                          # motion 3 failed
    info = sweep.eval_info()
    ks = range(1, U + 1)
    assert info["eval_mpjpe_all"] == pytest.approx(sum(2.0 * k * k for k in ks) / sum(2.0 * k for k in ks))       # not the mean of the per-motion means
    assert info["vel_dist"] == pytest.approx(sum(3.0 * k * k for k in ks if k != 4) / sum(1.0 * k for k in ks if k != 4))
    assert info["eval_mpjpe_succ"] == pytest.approx(sum(2.0 * k * k for k in ks if k != 4) / sum(2.0 * k for k in ks if k != 4))
    assert set(info) == {"eval_success_rate", "eval_mpjpe_all", "eval_mpjpe_succ", "accel_dist", "vel_dist", "mpjpel_all", "mpjpel_succ", "mpjpe_pa"}
    # nothing succeeded: "succ" falls back to "all"
    for m in sweep.terminate_memory:
        m[:] = True
    info = sweep.eval_info()
    assert info["eval_mpjpe_succ"] == info["eval_mpjpe_all"] and info["mpjpel_succ"] == info["mpjpel_all"]


def _reference_eval_bodies(humanoid_type, body_names):
    """The statements of Humanoid's setup that build ``_eval_bodies`` (humanoid.py:381-388), run on a stub that has the body names."""
    path = os.path.join(refload.REFERENCE_ROOT, "phc", "env", "tasks", "humanoid.py")
    src = open(path).read()
    cls = [n for n in ast.parse(src).body if isinstance(n, ast.ClassDef) and n.name == "Humanoid"][0]
    for fn in (n for n in cls.body if isinstance(n, ast.FunctionDef)):
        stmts = [s for s in fn.body if "_body_names_orig_copy" in (ast.get_source_segment(src, s) or "")]
        if stmts:
            break
    stub = types.SimpleNamespace(humanoid_type=humanoid_type, _body_names_orig=list(body_names))
    exec(compile(ast.Module(body=stmts, type_ignores=[]), "<reference:Humanoid._eval_bodies>", "exec"), {"self": stub})
    return list(stub._eval_bodies)


@pytest.mark.parametrize("humanoid", ["smpl", "smplx"])
def test_evaluation_bodies_are_the_reference_eval_bodies(request, humanoid):
    names = syn.skeleton(humanoid)["body_names"]
    with RefRecord(request) as R:
        want = R.obj("eval_bodies", lambda: _reference_eval_bodies(humanoid, names))
        assert eval_body_names(names, humanoid) == want
    assert len(want) == len(names) - (4 if humanoid == "smpl" else 2) and "L_Toe" not in want
