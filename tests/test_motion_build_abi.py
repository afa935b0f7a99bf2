"""GPU: the C ABI of pulse_motion_build (include/pulse_hip.h section 2b') -- the ctypes mirror has the C struct's size, every argument the
launcher refuses comes back as PULSE_ERR_INVALID_ARG with a message that names what is wrong (nothing is launched then), and the tensor
wrapper rejects CPU tensors, wrong dtypes and non-contiguous inputs."""
import ctypes

import pytest
import torch

from pulse_amd import _lib, kernels
from pulse_amd.env.motion_lib import MotionLib

pytestmark = pytest.mark.gpu
OK, INVALID = 0, -1


def _args(dev, j=3, frames=(2, 3), parents=(-1, 0, 1)):
    """A valid argument struct over tiny device buffers, and everything that must outlive it."""
    m, total = len(frames), sum(frames)
    offsets, stride, _ = MotionLib.record_layout(j)
    rot = torch.zeros(total, j, 4, device=dev)
    rot[..., 3] = 1.0
    nf = torch.tensor(frames, dtype=torch.int64)
    t = {"src_rot": rot, "src_trans": torch.zeros(total, 3, device=dev), "clip_src_start": (torch.cumsum(nf, 0) - nf).to(dev),
         "clip_out_start": torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(nf, 0)]).to(dev), "clip_dt": torch.full((m,), 1 / 30, device=dev),
         "local_translation": torch.zeros(m, j, 3, device=dev), "frames": torch.full((total, stride), float("nan"), device=dev)}
    host = {"nf": nf, "par": (ctypes.c_int32 * len(parents))(*parents)}
    a = _lib.MotionBuildArgs()
    for k, v in t.items():
        setattr(a, k, v.data_ptr())
    a.src_frames, a.num_clips, a.num_bodies = total, m, j
    a.clip_frames_host, a.parent_indices_host = nf.data_ptr(), ctypes.cast(host["par"], ctypes.c_void_p)
    a.total_frames, a.frame_stride = total, stride
    for k, v in offsets.items():
        setattr(a, "off_" + k, v)
    a.filter_w[:] = kernels.gaussian_weights()
    return a, t, host


def _call(a):
    lib = _lib.load()
    rc = lib.pulse_motion_build(ctypes.byref(a), None)
    m = lib.pulse_last_error()
    return rc, (m.decode() if m else "")


def test_struct_size_and_valid_call(dev):
    assert ctypes.sizeof(_lib.MotionBuildArgs) == _lib.load().pulse_sizeof_motion_build_args()
    a, t, _ = _args(dev)
    rc, m = _call(a)
    assert rc == OK, m
    torch.cuda.synchronize()
    assert torch.isfinite(t["frames"]).all()                     # every column written, the padding included
    assert _lib.load().pulse_motion_build(None, None) == INVALID


@pytest.mark.parametrize("what,needle", [("one_frame", "at least 2"), ("bodies_65", "not in [1,64]"), ("parent_ge_child", "precede"),
                                         ("root_parent", "root"), ("null_src_rot", "null"), ("null_frames", "null"), ("null_parents", "null"),
                                         ("null_clip_frames", "null"), ("misaligned", "16-byte aligned"), ("stride", "frame_stride"),
                                         ("overlap", "overlap"), ("quat_offset", "16-byte boundaries"), ("frame_sum", "total_frames")])
def test_refused_arguments(dev, what, needle):
    a, t, host = _args(dev)
    before = t["frames"].clone()
    if what == "one_frame":
        host["nf"][0], host["nf"][1] = 1, 4                      # same total: only the 1-frame clip is wrong
    elif what == "bodies_65":
        a.num_bodies = 65
    elif what == "parent_ge_child":
        host["par"][1] = 1
    elif what == "root_parent":
        host["par"][0] = 0
    elif what == "null_src_rot":
        a.src_rot = None
    elif what == "null_frames":
        a.frames = None
    elif what == "null_parents":
        a.parent_indices_host = None
    elif what == "null_clip_frames":
        a.clip_frames_host = None
    elif what == "misaligned":
        a.frames = t["frames"].data_ptr() + 4
    elif what == "stride":
        a.frame_stride = a.frame_stride - 2
    elif what == "overlap":
        a.off_gvs = a.off_gts
    elif what == "quat_offset":
        a.off_gts, a.off_grs, a.off_lrs = 0, 9, 21              # [gts | grs | lrs | ...] still tiles the record: only the alignment is wrong
    elif what == "frame_sum":
        a.total_frames = a.total_frames - 1
    rc, m = _call(a)
    assert rc == INVALID and needle in m, (what, rc, m)
    torch.cuda.synchronize()
    assert torch.equal(before.view(torch.int32), t["frames"].view(torch.int32)), "a refused call wrote records"


def test_wrapper_rejects_bad_tensors(dev):
    _, t, host = _args(dev)
    offsets = MotionLib.record_layout(3)[0]
    good = dict(src_rot=t["src_rot"], src_trans=t["src_trans"], clip_src_start=t["clip_src_start"], clip_out_start=t["clip_out_start"],
                clip_frames=host["nf"], clip_dt=t["clip_dt"], local_translation=t["local_translation"], parents=[-1, 0, 1])
    kernels.motion_build(t["frames"], offsets, **good)
    with pytest.raises(TypeError, match="CUDA tensor"):
        kernels.motion_build(t["frames"], offsets, **dict(good, src_rot=t["src_rot"].cpu()))
    with pytest.raises(TypeError, match="CUDA tensor"):
        kernels.motion_build(t["frames"].cpu(), offsets, **good)
    with pytest.raises(TypeError, match="dtype"):
        kernels.motion_build(t["frames"], offsets, **dict(good, src_rot=t["src_rot"].double()))
    with pytest.raises(TypeError, match="dtype"):
        kernels.motion_build(t["frames"], offsets, **dict(good, clip_out_start=t["clip_out_start"].int()))
    with pytest.raises(TypeError, match="CPU tensor"):
        kernels.motion_build(t["frames"], offsets, **dict(good, clip_frames=host["nf"].to(dev)))
    with pytest.raises(ValueError, match="contiguous"):
        kernels.motion_build(t["frames"], offsets, **dict(good, src_trans=torch.zeros(5, 6, device=dev)[:, :3]))
    with pytest.raises(ValueError, match="shape"):
        kernels.motion_build(t["frames"], offsets, **dict(good, clip_dt=t["clip_dt"][:1]))
