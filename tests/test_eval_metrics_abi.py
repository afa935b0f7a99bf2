"""CPU: the C ABI of pulse_im_eval_accum (include/pulse_hip.h section 2b'').  The ctypes mirror has the C struct's size, and every
argument the launcher refuses comes back as PULSE_ERR_INVALID_ARG with a message that names what is wrong, before anything touches the
device: no kernel is launched here (the pointers are host addresses that are never dereferenced)."""
import ctypes

import pytest

from pulse_amd import _lib

OK, INVALID = 0, -1


def _args(j=24, n=5):
    buf = (ctypes.c_double * 64)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a = _lib.ImEvalArgs()
    a.rb, a.rb_env_stride, a.ref_pos, a.ref_env_stride = base, 13 * j, base, 3 * j
    a.num_envs, a.num_bodies, a.num_steps, a.step = n, j, base, 0
    a.ring, a.accum, a.accum_stride = base, base, 8
    return a, buf


def _call(a):
    lib = _lib.load()
    rc = lib.pulse_im_eval_accum(ctypes.byref(a) if a is not None else None, None)
    m = lib.pulse_last_error()
    return rc, (m.decode() if m else "")


def test_struct_size_null_args_and_empty_problem():
    lib = _lib.load()
    assert ctypes.sizeof(_lib.ImEvalArgs) == lib.pulse_sizeof_im_eval_args()
    rc, m = _call(None)
    assert rc == INVALID and "null args" in m
    a, _ = _args(n=0)
    a.rb = None                                                   # no envs: a no-op whatever the pointers
    assert _call(a)[0] == OK


@pytest.mark.parametrize("what,needle", [("null_rb", "null rb"), ("null_ref", "null ref_pos"), ("null_num_steps", "null num_steps"),
                                         ("null_ring", "null ring"), ("null_accum", "null accum"), ("bodies_65", "not in [1,64]"),
                                         ("bodies_0", "not in [1,64]"), ("short_rb_pitch", "rb_env_stride"), ("short_ref_pitch", "ref_env_stride"),
                                         ("short_accum_pitch", "accum_stride"), ("negative_step", "negative step"), ("negative_envs", "negative num_envs"),
                                         ("misaligned_accum", "8-byte aligned"), ("misaligned_rb", "4-byte aligned")])
def test_refused_arguments(what, needle):
    a, keep = _args()
    if what == "null_rb":
        a.rb = None
    elif what == "null_ref":
        a.ref_pos = None
    elif what == "null_num_steps":
        a.num_steps = None
    elif what == "null_ring":
        a.ring = None
    elif what == "null_accum":
        a.accum = None
    elif what == "bodies_65":
        a.num_bodies, a.rb_env_stride, a.ref_env_stride = 65, 13 * 65, 3 * 65
    elif what == "bodies_0":
        a.num_bodies = 0
    elif what == "short_rb_pitch":
        a.rb_env_stride = 13 * 24 - 1
    elif what == "short_ref_pitch":
        a.ref_env_stride = 3 * 24 - 1
    elif what == "short_accum_pitch":
        a.accum_stride = 7
    elif what == "negative_step":
        a.step = -1
    elif what == "negative_envs":
        a.num_envs = -2
    elif what == "misaligned_accum":
        a.accum = a.accum + 4
    elif what == "misaligned_rb":
        a.rb = a.rb + 2
    rc, m = _call(a)
    assert rc == INVALID and needle in m, (what, rc, m)
