"""Host time of one kernel launch wrapper, without a GPU: _lib.launch beside the hand-written form it replaced (device guard, one
_lib.ptr per tensor, the stream, _lib.check), for a plain call with ten arguments and for a struct call with fourteen fields.  The
library is a stub that returns 0, the stream a constant; CPU tensors.   python tools/launch_path_host_time.py"""
import ctypes
import os
import sys
import timeit

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import e3dge_amd  # noqa: F401,E402
from e3dge_amd import _lib  # noqa: E402


def us(fn, n=20000):
    return 1e6 * min(timeit.repeat(fn, number=n, repeat=7)) / n


class _Stub:
    e3dge_plain = e3dge_struct = staticmethod(lambda *a: 0)


class _PlainArgs(ctypes.Structure):          # the mirror as it was: no tensor fields
    _fields_ = _lib.SirenBwdArgs._fields_


_lib._lib, _lib.stream_of = _Stub(), lambda t: 0
t = [torch.zeros(4) for _ in range(9)]
p = _lib.ptr


def old_plain():
    with _lib.on_device(t[0].device):
        rc = _lib.load().e3dge_plain(p(t[0]), p(t[1]), p(t[2]), p(None), 1.5, 2, 1000, p(t[3]), p(t[4]), 3, _lib.stream_of(t[0]))
    _lib.check(rc, "e3dge_plain")


def old_struct():
    a = _PlainArgs(packed=p(t[0]), film=p(t[1]), args=p(t[2]), d_feat=p(t[3]), d_rgb=p(None), d_sdf=p(t[4]), wg=p(t[5]), wb=p(t[6]),
                   batch=2, precision=3, n_pts=1000, box_scale=1.5, partials=p(t[7]), dfilm=p(t[8]))
    with _lib.on_device(t[0].device):
        rc = _lib.load().e3dge_struct(ctypes.byref(a), _lib.stream_of(t[0]))
    _lib.check(rc, "e3dge_struct")


def new_struct():
    _lib.launch("e3dge_struct", _lib.SirenBwdArgs(packed=t[0], film=t[1], args=t[2], d_feat=t[3], d_rgb=None, d_sdf=t[4], wg=t[5], wb=t[6],
                                                  batch=2, precision=3, n_pts=1000, box_scale=1.5, partials=t[7], dfilm=t[8]))


new_plain = lambda: _lib.launch("e3dge_plain", t[0], t[1], t[2], None, 1.5, 2, 1000, t[3], t[4], 3)
print(f"plain call, ten arguments:    hand-written {us(old_plain):.2f} us, _lib.launch {us(new_plain):.2f} us")
print(f"struct call, fourteen fields: hand-written {us(old_struct):.2f} us, _lib.launch {us(new_struct):.2f} us")
