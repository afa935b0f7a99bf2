"""Every GEMM launch the training agents issue, judged against the fp64 model of its descriptor (oracle/gemm_ref.py).

The descriptor builders (make_gemm_desc / make_gemm_x3p_desc) are wrapped so every descriptor remembers the tensors its pointers came from,
and the two launchers (launch_gemm / launch_gemm_x3p: Plan.run goes through them too) are wrapped so the FIRST launch of each distinct
descriptor (keyed by the struct's bytes) is audited: every extent the launch reads or writes must lie inside the storage its pointer came
from, the inputs are snapshot to fp64, the written rectangles are poisoned with NaN (unless they overlap an input), the launch runs on the
caller's stream, and every output is judged: per-element bound, aggregate rule against an fp32 yardstick, bf16 / mask / plane / split-K
rules.  One train_epoch (mini_epochs = 1) per agent; each case also asserts its own coverage so a hook that audits nothing fails.
"""
import time

import pytest
import torch

from oracle import gemm_ref as GR
from pulse_amd import _lib, configs
from pulse_amd import kernels as K

pytestmark = pytest.mark.gpu

NAN16 = 0x7FC0            # bf16 quiet NaN (int16 bit pattern)


class Auditor:
    def __init__(self):
        self.owners = {}          # id(desc) -> (desc, {field: tensor})
        self.seen = set()
        self.rows = []            # one dict per audited launch
        self.phase = "rollout"
        self.failures = []

    # ------------------------------------------------------------------ descriptor builders
    def wrap_make(self, orig, kind):
        def make(A, B, *args, **kw):
            d, fl, tag = orig(A, B, *args, **kw)
            t = {"A": A, "B": B}
            if kind == "f32":
                t["C"] = args[0] if args else kw.get("C")
                for f in ("C2", "bias", "aux", "rowsum", "relu_mask"):
                    t[f] = kw.get(f)
            else:
                for f in ("C", "Cp", "C2", "bias", "aux", "out_colsum", "relu_mask8"):
                    t[f] = kw.get(f)
            self.owners[id(d)] = (d, {k: v for k, v in t.items() if v is not None})
            return d, fl, tag
        return make

    # ------------------------------------------------------------------ launchers
    def wrap_launch(self, orig, kind):
        def launch(d, flops=0.0, tag="fwd", stream=None):
            key = (kind, bytes(d))
            if key in self.seen:
                return orig(d, flops, tag, stream)
            self.seen.add(key)
            return self.audit(orig, kind, d, flops, tag, stream)
        return launch

    def audit(self, orig, kind, d, flops, tag, stream):
        torch.cuda.synchronize()
        assert id(d) in self.owners and self.owners[id(d)][0] is d, f"{tag}: descriptor not built by make_gemm_desc / make_gemm_x3p_desc"
        tens = self.owners[id(d)][1]
        regions = GR.f32_regions(d) if kind == "f32" else GR.x3p_regions(d)
        flat = {}
        for name, (ptr, es, n, out) in regions.items():
            t = tens.get(name)
            assert t is not None, f"{tag}: pointer {name} has no tensor behind it"
            st = t.untyped_storage()
            lo, hi = ptr, ptr + es * n
            assert st.data_ptr() <= lo and hi <= st.data_ptr() + st.nbytes(), (
                f"{tag} M={d.M} N={d.N} K={d.K}: {name} extent [{lo - st.data_ptr()}, {hi - st.data_ptr()}) bytes past the storage of "
                f"{st.nbytes()} bytes")
            dt = {4: torch.float32, 2: torch.int16, 1: torch.uint8}[es]
            if name == "relu_mask":
                dt = torch.int32
            whole = torch.empty(0, dtype=dt, device=t.device).set_(st, 0, (st.nbytes() // es,), (1,))
            assert (lo - st.data_ptr()) % es == 0
            off = (lo - st.data_ptr()) // es
            flat[name] = whole[off:off + max(n, 1)]
        ins = {k: v for k, v in flat.items() if not regions[k][3]}
        mem = {}
        for k, v in ins.items():
            if v.dtype == torch.int16 and not (k == "aux" and kind == "x3p" and not d.aux_is_bf16):
                mem[k] = GR.bf16_bits_to_f64(v)
            elif v.dtype in (torch.int32, torch.uint8):
                mem[k] = v.clone()
            else:
                mem[k] = v.double()
        # poison the written rectangles (not if they overlap an input: in place)
        in_ranges = [(regions[k][0], regions[k][0] + regions[k][1] * regions[k][2]) for k in ins]
        for name, (shape, strides, off) in GR.output_rects(d, kind).items():
            ptr, es, n, _ = regions[name]
            if any(a < ptr + es * n and ptr < b for a, b in in_ranges):
                continue
            v = GR.view(flat[name], shape, strides, off)
            v.fill_(NAN16 if v.dtype == torch.int16 else float("nan"))
        if "relu_mask" in flat and regions["relu_mask"][3]:
            flat["relu_mask"].fill_(0x5A5A5A5A)
        if "relu_mask8" in flat and regions["relu_mask8"][3]:
            flat["relu_mask8"].fill_(0xA5)
        orig(d, flops, tag, stream)
        torch.cuda.synchronize()
        tile = _lib.load().pulse_gemm_last_tile() if kind == "f32" else 0
        outs = {k: v for k, v in flat.items() if regions[k][3]}
        rep = GR.judge(d, kind, mem, outs)
        form = ("fwd" if d.b_layout == GR.RED else "dx") if d.a_layout == GR.RED else "dw"
        row = {"kind": kind, "tag": tag, "form": form, "phase": self.phase, "M": d.M, "N": d.N, "K": d.K, "batch": d.batch, "split": d.split_k,
               "epi": d.epilogue, "act": d.activation, "tile": tile, "worst": rep["worst"], "agg": rep["agg"] * GR.RHO, "yard": rep["yard"],
               "compute": getattr(d, "compute_type", -1), "planes": getattr(d, "planes", 0)}
        self.rows.append(row)
        print(f"[audit] {self.phase:7s} {kind:3s} {tag:9s} M={d.M:5d} N={d.N:5d} K={d.K:5d} b={d.batch} split={d.split_k} layouts=({d.a_layout},{d.b_layout}) "
              f"epi={d.epilogue} act={d.activation} tile={tile:3d} worst err/tol={rep['worst']:.3g} rms/yardstick={rep['agg'] * GR.RHO:.3g}")
        if rep["problems"]:
            self.failures.append(f"{tag} M={d.M} N={d.N} K={d.K} batch={d.batch} split={d.split_k}: " + "; ".join(rep["problems"]))


@pytest.fixture
def auditor(monkeypatch):
    a = Auditor()
    monkeypatch.setattr(K, "make_gemm_desc", a.wrap_make(K.make_gemm_desc, "f32"))
    monkeypatch.setattr(K, "make_gemm_x3p_desc", a.wrap_make(K.make_gemm_x3p_desc, "x3p"))
    monkeypatch.setattr(K, "launch_gemm", a.wrap_launch(K.launch_gemm, "f32"))
    monkeypatch.setattr(K, "launch_gemm_x3p", a.wrap_launch(K.launch_gemm_x3p, "x3p"))
    assert not torch.backends.cuda.matmul.allow_tf32
    yield a
    for k in range(16):
        if k != 7:
            K.gemm_set_option(k, 0)


# name: make_agent arguments, F32_MODE, minimum audited launches, pulse_gemm_f32 tiles that must be seen (64 / 128 = gemm_x3<.., 1 / 2>,
# 96 = gemm_x3s, 256 = gemm_x3w; the fp32 MFMA kernel reports 128), whether the weight gradients go through split-K slabs
CASES = {
    "cfg1": (dict(name="cfg1"), "x3", 12, {128}, False),
    "cfg2": (dict(name="cfg2"), "x3", 12, {256, 128, 96, 64}, True),
    "cfg2_mfma32": (dict(name="cfg2"), "mfma32", 12, {128}, True),
    "cfg2_shard": (dict(name="cfg2", num_envs_override=512, minibatch_size=2048), "x3", 12, {256, 128, 64}, True),
    "cfg3": (dict(name="cfg3"), "x3", 45, {256, 128, 64}, True),
    "cfg3_ppo": (dict(name="cfg3_ppo"), "x3", 55, {256, 128, 64}, True),
    "cfg5": (dict(name="cfg5"), "x3", 20, set(), True),
    "cfg5_f32": (dict(name="cfg5_f32"), "x3", 25, {256, 128, 96, 64}, True),
    "speed_z": (dict(name="speed_z"), "x3", 22, {256, 128, 96, 64}, True),
    "terrain_z": (dict(name="terrain_z"), "x3", 40, {256, 128, 64}, True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_every_launch_of_an_epoch_matches_the_fp64_model(dev, auditor, monkeypatch, case):
    kw, mode, min_launches, tiles, split_dw = CASES[case]
    monkeypatch.setattr(K, "F32_MODE", mode)
    t0 = time.time()
    torch.manual_seed(7)
    kw = dict(kw)
    agent, _ = configs.make_agent(kw.pop("name"), device=str(dev), seed=7, mini_epochs=1, **kw)
    play = agent.play_steps

    def play_steps():
        auditor.phase = "rollout"
        try:
            return play()
        finally:
            auditor.phase = "update"
    monkeypatch.setattr(agent, "play_steps", play_steps)
    agent.train_epoch()
    torch.cuda.synchronize()
    rows = auditor.rows
    f32 = [r for r in rows if r["kind"] == "f32"]
    seen_tiles = {r["tile"] for r in f32}
    worst = max((r["worst"] for r in rows), default=0.0)
    agg = max((r["agg"] for r in rows), default=0.0)
    print(f"[audit-summary] {case}: {len(rows)} launches audited ({len(f32)} pulse_gemm_f32, {len(rows) - len(f32)} pulse_gemm_x3p), tiles "
          f"{sorted(seen_tiles)}, worst err/tol {worst:.3g}, worst rms/yardstick {agg:.3g}, {time.time() - t0:.1f} s")
    assert not auditor.failures, "\n".join(auditor.failures[:20])
    assert len(rows) >= min_launches
    assert tiles <= seen_tiles, f"tiles seen {sorted(seen_tiles)}, expected at least {sorted(tiles)}"
    phases = {(r["phase"], r["form"]) for r in rows}
    assert ("rollout", "fwd") in phases and ("update", "fwd") in phases and ("update", "dx") in phases and ("update", "dw") in phases, phases
    assert not split_dw or any(r["split"] > 1 for r in rows if r["form"] == "dw"), "no split-K weight-gradient launch was audited"
    if case == "cfg5":                                # bf16 storage: the update runs on the single-plane kernels
        assert any(r["kind"] == "x3p" and r["planes"] == 1 for r in rows)
    else:
        want = GR.COMPUTE_F32X3 if mode == "x3" else GR.COMPUTE_F32
        assert all(r["compute"] == want for r in f32), {r["compute"] for r in f32}
