"""Host side of the layout tests (DESIGN.md 'What a kernel may be handed'): the variants of tests/layout_variants.py have the
properties their names promise, `_lib.dense` returns what a kernel may take, and the entry names the package launches can be listed
from its source (the GPU side, tests/test_gpu_layouts.py, compares that list with what its gate saw)."""
import os
import re

import pytest
import torch

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib

import layout_variants as lv

SHAPES = [(2, 5, 6, 4), (2, 5, 3, 3), (2, 125, 3), (200, 301), (1, 3, 31, 31), (7,)]


def _x(shape, dtype=torch.float32):
    n = 1
    for s in shape:
        n *= s
    return (torch.arange(n, dtype=torch.float64).reshape(shape) * 0.37 - 3.0).to(dtype)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_variant_equals_its_dense_twin_and_sits_in_sentinels(shape):
    x = _x(shape)
    kinds = lv.kinds_for(x)
    assert "offset4" in kinds and "expanded1" not in kinds
    if lv.applies(x, "expanded1"):
        kinds = kinds + ["expanded1"]
    for kind in kinds:
        v = lv.Variant(x, kind)
        t, twin = v.tensor, lv.dense_twin(x, kind)
        assert t.shape == x.shape and twin.is_contiguous()
        assert torch.equal(t, twin), kind
        if not kind.startswith("expanded"):
            assert torch.equal(twin, x)
        # what the view does not cover is sentinel, what it covers is not (the values above never equal SENTINEL)
        assert bool((v.buffer[~v.mask] == lv.SENTINEL).all()) and int((~v.mask).sum()) > 0, kind
        assert not bool((v.buffer[v.mask] == lv.SENTINEL).any()), kind
        covered = {"expanded": x.numel() // x.shape[0], "expanded1": x.numel() // x.shape[min(1, x.ndim - 1)]}.get(kind, x.numel())
        assert int(v.mask.sum()) == covered, kind
        assert v.buffer.data_ptr() % 16 == 0
        v.check_untouched()


def test_variant_properties():
    x4, x3, x2 = _x((2, 5, 6, 4)), _x((2, 125, 3)), _x((200, 301))
    t = lv.variant(x3, "offset4")
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    t = lv.variant(x2, "pitch")
    assert t.stride() == (301 + lv.PITCH_PAD, 1) and not t.is_contiguous()
    t = lv.variant(x4, "pitch")
    assert t.stride(-1) == 1 and t.stride(-2) == 4 + lv.PITCH_PAD and not t.is_contiguous()
    t = lv.variant(x4, "channels_last")
    assert t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous() and t.data_ptr() % 16 == 0
    t = lv.variant(x3, "permuted")
    assert t.stride() == (375, 1, 125) and t.data_ptr() % 16 == 0
    assert lv.variant(x2, "permuted").stride() == (1, 200)
    t = lv.variant(x4, "wide")
    assert t.stride() == (7 * 24, 24, 4, 1) and t.storage_offset() == 24 and not t.is_contiguous()
    t = lv.variant(x3, "expanded")
    assert t.stride() == (0, 3, 1) and torch.equal(t[0], t[1]) and torch.equal(t[0], x3[0])
    t = lv.variant(x3, "expanded1")
    assert t.stride() == (3, 0, 1) and torch.equal(t[:, 7], x3[:, 0]) and torch.equal(t, lv.dense_twin(x3, "expanded1"))
    assert not lv.applies(x3, "channels_last") and not lv.applies(x4, "permuted") and not lv.applies(_x((1, 3, 4, 4)), "expanded")
    assert not lv.applies(_x((2, 1, 4, 4)), "channels_last")          # (one channel: NHWC is the dense layout)
    assert lv.kinds_for(_x((7,))) == ["offset4", "expanded"]
    with pytest.raises(ValueError):
        lv.variant(x3, "channels_last")


def test_check_untouched_sees_a_write_to_the_view_and_to_a_sentinel():
    x = _x((2, 5, 6, 4))
    for kind in lv.kinds_for(x):
        v = lv.Variant(x, kind)
        v.buffer.view(-1)[-1] += 1.0                 # a sentinel (every carving leaves the buffer's last element outside the view)
        assert not bool(v.mask.view(-1)[-1])
        with pytest.raises(AssertionError):
            v.check_untouched()
        v = lv.Variant(x, kind)
        v.buffer[v.mask] += 1.0
        with pytest.raises(AssertionError):
            v.check_untouched()


def test_dense_returns_the_tensor_or_an_aligned_contiguous_copy():
    x = _x((2, 125, 3))
    assert _lib.dense(None) is None
    assert x.data_ptr() % 16 == 0 and _lib.dense(x) is x
    for kind in lv.kinds_for(x):
        t = lv.variant(x, kind)
        d = _lib.dense(t)
        assert d is not t and d.is_contiguous() and d.data_ptr() % 16 == 0 and torch.equal(d, t), kind
        assert d.untyped_storage().data_ptr() != t.untyped_storage().data_ptr()
    sl = x[1:]                                       # contiguous, so .contiguous() is a no-op, and 1500 bytes into the block
    assert sl.is_contiguous() and sl.contiguous() is sl and sl.data_ptr() % 16 == 12
    d = _lib.dense(sl)
    assert d is not sl and d.data_ptr() % 16 == 0 and torch.equal(d, sl)
    assert _lib.dense(sl, align=4) is sl
    e = torch.empty(0)
    assert _lib.dense(e) is e
    cl = lv.variant(_x((2, 1, 4, 4)), "wide")        # a copy keeps the logical order, never the source's memory format
    assert _lib.dense(cl).stride() == (16, 16, 4, 1)


def launched_entry_names():
    """Every e3dge_* name the package source hands to _lib.launch / _lib.query: the string literals of the package outside _lib.py (two
    call sites pass the name in a variable, and two append a dtype suffix, so the literals are taken wherever they stand), kept when the
    binding declares them.  A literal followed by `+` is a family: its suffixed members count as the same row."""
    pkg = os.path.dirname(os.path.abspath(_lib.__file__))
    names, families = set(), set()
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py") and f != "_lib.py":
                src = open(os.path.join(root, f)).read()
                for m in re.finditer(r'"(e3dge_\w+)"(\s*\+)?', src):
                    (families if m.group(2) else names).add(m.group(1))
    return names, families


def test_the_launched_entries_can_be_listed_from_the_source():
    names, families = launched_entry_names()
    assert families == {"e3dge_fused_bias_act", "e3dge_upfirdn2d"}
    unknown = sorted(n for n in names | families if n not in _lib.SIGNATURES)
    assert not unknown, f"names in the package source that the binding does not declare: {unknown}"
    assert {"e3dge_local_query", "e3dge_avgpool_fwd", "e3dge_lpips_forward", "e3dge_siren_render_fwd"} <= names
    assert len(names) > 60


def test_the_lists_of_the_gpu_test_name_real_entries_and_real_lines():
    """FOUR_BYTE_OK / TAKES_STRIDES / NOT_REACHED of tests/test_gpu_layouts.py: every key is a declared entry with that many arguments or
    a field of a declared argument struct, and every `file.hip:line` a justification cites exists."""
    import test_gpu_layouts as g
    csrc = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
    for key in list(g.FOUR_BYTE_OK) + list(g.TAKES_STRIDES):
        owner, what = key
        if isinstance(what, int):
            assert owner in _lib.SIGNATURES and what < len(_lib.SIGNATURES[owner][1]), key
        else:
            assert what in dict(getattr(_lib, owner)._fields_), key
    for key, why in g.FOUR_BYTE_OK.items():
        cited = re.findall(r"(\w+\.(?:hip|h)):(\d+)", why)
        assert cited, (key, why)                                     # every item carries the file:line of the access or branch
        for name, line in cited:
            with open(os.path.join(csrc, name)) as f:
                lines = f.readlines()
            assert int(line) <= len(lines), (key, why)
            text = lines[int(line) - 1]
            # the cited line is a load through an index or a dereference, an alignment branch, or the 4-byte-aligned vector type
            assert re.search(r"\w\[|\*\w|aligned|& 15|F4[uU]\b|WgU4", text), (key, name, line, text.strip())
    for (owner, what), spec in g.TAKES_STRIDES.items():
        if isinstance(spec, int):
            assert spec < len(_lib.SIGNATURES[owner][1])
        elif spec is not g.ROWS16:
            assert spec in dict(getattr(_lib, owner)._fields_), (owner, what, spec)
    names, families = launched_entry_names()
    assert set(g.NOT_REACHED) <= names | families and all(g.NOT_REACHED.values())
    assert len({r.name for r in g.ROWS}) == len(g.ROWS) >= 47
