"""CPU: the one launch path of the package (_lib.launch and the tensor-accepting argument structs), against a recording stub in
place of the loaded library; and the scan that keeps hand-written launch sites out of the package."""
import ctypes
import glob
import os

import pytest
import torch

from conftest import REPO

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib

STREAM = 0x5EED


class _Recorder:
    """Stands in for the ctypes handle: every e3dge_* attribute is a function that records its arguments and returns `rc`."""

    def __init__(self, rc=0, message=b"stub says no"):
        self.calls, self.rc, self.message, self.guards = [], rc, message, []

    def e3dge_last_error(self):
        return self.message

    def __getattr__(self, name):
        if not name.startswith("e3dge_"):
            raise AttributeError(name)
        return lambda *args: (self.calls.append((name, args)), self.rc)[1]


@pytest.fixture
def stub(monkeypatch):
    rec = _Recorder()

    class guard:
        def __init__(self, dev):
            self.dev = dev

        def __enter__(self):
            rec.guards.append(("enter", self.dev, len(rec.calls)))

        def __exit__(self, *exc):
            rec.guards.append(("exit", self.dev, len(rec.calls)))
            return False

    monkeypatch.setattr(_lib, "_lib", rec)                      # load() returns the handle it already has
    monkeypatch.setattr(_lib, "stream_of", lambda t: STREAM)
    monkeypatch.setattr(_lib, "on_device", guard)
    return rec


def test_launch_converts_arguments_and_appends_the_stream(stub):
    a, b = torch.zeros(4), torch.zeros(3, dtype=torch.int32)
    s = _lib.SirenBwdArgs(packed=a, batch=2)
    _lib.launch("e3dge_anything", a, None, s, 7, 1.5, b, a.data_ptr() + 8)
    (name, args), = stub.calls
    assert name == "e3dge_anything" and len(args) == 8
    assert args[0] == a.data_ptr() and args[1] is None
    assert args[2]._obj is s                                    # ctypes.byref(s): the struct itself, not a copy
    assert args[3] == 7 and type(args[3]) is int and args[4] == 1.5 and type(args[4]) is float
    assert args[5] == b.data_ptr() and args[6] == a.data_ptr() + 8
    assert args[7] == STREAM
    # the call ran inside the guard of the first tensor's device
    assert stub.guards == [("enter", a.device, 0), ("exit", a.device, 1)]


def test_launch_takes_the_device_from_a_struct_when_no_tensor_is_passed(stub):
    a = torch.zeros(4)
    _lib.launch("e3dge_anything", _lib.WsLinear(x=a, n_rows=1))
    assert stub.guards[0] == ("enter", a.device, 0) and stub.calls[0][1][1] == STREAM
    with pytest.raises(RuntimeError, match="e3dge_anything"):   # nothing to take a device from
        _lib.launch("e3dge_anything", _lib.WsLinear(n_rows=1), 3)
    assert len(stub.calls) == 1


@pytest.mark.parametrize("cls", [_lib.RenderArgs, _lib.RenderBwdArgs, _lib.SirenBwdArgs, _lib.SirenWgradArgs, _lib.ModconvArgs,
                                 _lib.Dec2Plan, _lib.Dec2BwdPlan, _lib.WsLinear, _lib.Wgrad, _lib.MeshRenderArgs, _lib.NoiseProjectArgs])
def test_structs_accept_tensors_for_pointer_fields(cls):
    ptrs = [n for n, t in cls._fields_ if t is ctypes.c_void_p]
    nums = [n for n, t in cls._fields_ if t in (ctypes.c_int, ctypes.c_int64, ctypes.c_float)]
    assert ptrs and nums
    ts = {n: torch.zeros(i + 1) for i, n in enumerate(ptrs)}
    ts[ptrs[-1]] = None
    by_tensor = cls(**ts, **{n: i + 1 for i, n in enumerate(nums)})
    by_pointer = cls(**{n: _lib.ptr(t) for n, t in ts.items()}, **{n: i + 1 for i, n in enumerate(nums)})
    assert bytes(by_tensor) == bytes(by_pointer)
    assert getattr(by_tensor, ptrs[0]) == ts[ptrs[0]].data_ptr() and getattr(by_tensor, ptrs[-1]) is None
    # later assignment: a tensor, None, a plain address, a number
    late, other = cls(), torch.zeros(5)
    for n, t in ts.items():
        setattr(late, n, t)
    for i, n in enumerate(nums):
        setattr(late, n, i + 1)
    assert bytes(late) == bytes(by_pointer)
    setattr(late, ptrs[0], other)
    setattr(by_pointer, ptrs[0], other.data_ptr())
    assert bytes(late) == bytes(by_pointer)
    setattr(late, ptrs[0], None)
    assert getattr(late, ptrs[0]) is None
    assert ctypes.sizeof(cls) == ctypes.sizeof(type("Plain", (ctypes.Structure,), {"_fields_": cls._fields_}))


def test_nested_structs_accept_tensors_and_report_to_the_plan():
    plan, t = _lib.Dec2Plan(), torch.zeros(4)
    plan.up[2].wpre, plan.rgb1.out = t, t
    assert plan.up[2].wpre == t.data_ptr() and plan.rgb1.out == t.data_ptr() and plan.up[1].wpre is None
    assert plan.devices == [t.device]
    plan.conv[0].noise = torch.empty(2, device="meta")
    assert len(plan.devices) == 2


def test_failing_call_raises_with_the_symbol_and_the_library_message(stub):
    stub.rc = -1
    with pytest.raises(RuntimeError) as e:
        _lib.launch("e3dge_siren_tangent_tr", torch.zeros(2), 3)
    assert "e3dge_siren_tangent_tr" in str(e.value) and "stub says no" in str(e.value) and "-1" in str(e.value)
    assert len(stub.calls) == 1


def test_tensor_on_a_second_device_raises_before_anything_is_queued(stub):
    here, there = torch.zeros(4), torch.empty(4, device="meta")
    with pytest.raises(RuntimeError, match="e3dge_pos_encoding"):
        _lib.launch("e3dge_pos_encoding", here, 4, 0, there, 1, 7)
    with pytest.raises(RuntimeError, match="e3dge_siren_bwd"):
        _lib.launch("e3dge_siren_bwd", _lib.SirenBwdArgs(packed=here, film=there, batch=1))
    late = _lib.SirenBwdArgs(packed=here, batch=1)
    late.d_lin = there
    with pytest.raises(RuntimeError, match="e3dge_siren_bwd"):
        _lib.launch("e3dge_siren_bwd", late)
    with pytest.raises(RuntimeError, match="e3dge_wgrad"):      # a struct on one device, a tensor beside it on another
        _lib.launch("e3dge_wgrad", _lib.Wgrad(a=here), there)
    assert stub.calls == [] and stub.guards == []


def test_package_has_no_hand_written_launch_sites():
    """Every kernel launch of the package goes through _lib.launch: outside _lib.py no device guard of torch's, no _lib.check, no
    ctypes.byref and no _lib.ptr is spelled out."""
    pkg = os.path.join(REPO, "cvpr23-e3dge_amd")
    files = [f for f in glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True) if os.path.basename(f) != "_lib.py"]
    assert len(files) >= 12
    hits = []
    for f in files:
        for i, line in enumerate(open(f).read().splitlines(), 1):
            hits += [f"{os.path.relpath(f, REPO)}:{i}: {s}" for s in ("torch.cuda.device(", "_lib.check(", "ctypes.byref(", "_lib.ptr(") if s in line]
    assert not hits, "\n".join(hits)
