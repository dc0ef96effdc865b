"""GPU: the rows of the trainable 2-D residual aligner for the layouts table of tests/test_gpu_layouts.py -- forward + backward of the
autograd node (e3dge_amd.alignment._AlignerNode) in the eval and the train form and through align(), with every input and the upstream
gradient in every layout of tests/layout_variants.py, all of them together, and on a side stream; bit for bit the dense run's results,
inputs untouched, no output in an input's buffer, every pointer as the gate of that file wants it.

The rows are appended to that file's ROWS / BY_NAME when this file is imported, so that its engine (_check_case, the gate) runs them
and its coverage test (test_every_launched_entry_has_a_row_or_a_reason) drives the new entries through its own gate: the table is
extended from here because this file is new and that one is not.  Running that file without this one leaves the coverage test without
these rows."""
import pytest
import torch

import e3dge_amd  # noqa: F401
import test_gpu_layouts as table
from test_gpu_layouts import DEV, Row, _bits_equal, _check_case, _device_inputs, _leaf, _reference, gate  # noqa: F401  (gate: autouse here too)

pytestmark = pytest.mark.gpu
WATCHED = ("conv_layer1.0.weight", "dconv_layer1.0.res_layer.0.bias", "conv_layer3.1.res_layer.2.weight", "dconv_layer3.2.res_layer.4.weight")


def _inputs():
    from test_aligner_host import aligner_input
    x = aligner_input(1, 5)
    return dict(x=x, res_gt=x[:, :3].contiguous(), thumb=x[:, 3:, ::4, ::4].contiguous(), g=table._rand(77, 1, 3, 256, 256))


def _state(train):
    def build():
        from test_gpu_aligner_bwd import new_trainable
        return new_trainable(train)
    return build


def _grads(m, out, leaves, g):
    named = dict(m.named_parameters())
    grads = torch.autograd.grad(out, list(leaves) + [named[k] for k in WATCHED], g)
    return dict(out=out.detach(), **{f"g_input{i}": grads[i] for i in range(len(leaves))}, **{"g_" + k: v for k, v in zip(WATCHED, grads[len(leaves):])})


def _node_run(m, t):
    from e3dge_amd.alignment import _AlignerNode
    x = _leaf(t["x"])
    _AlignerNode.branches = []                                       # (the debug record of the PReLU branches is an output of this row)
    try:
        out = m(x)
        branch = _AlignerNode.branches[0]
    finally:
        _AlignerNode.branches = None
    return dict(_grads(m, out, [x], t["g"]), branch=branch)


def _align_run(m, t):
    res_gt, thumb = _leaf(t["res_gt"]), _leaf(t["thumb"])
    return _grads(m, m.align(res_gt, thumb), [res_gt, thumb], t["g"])


NODE = {"e3dge_aligner_forward_saving", "e3dge_aligner_backward"}
ROWS = [
    Row("aligner_node_eval", _inputs, _node_run, NODE | {"e3dge_aligner_branch_bytes"}, _state(False), upstream={"g"}, fixed={"res_gt", "thumb"}),
    Row("aligner_node_train", _inputs, _node_run, NODE | {"e3dge_aligner_branch_bytes"}, _state(True), upstream={"g"}, fixed={"res_gt", "thumb"}),
    Row("aligner_node_align_eval", _inputs, _align_run, NODE, _state(False), upstream={"g"}, fixed={"x"}),
    Row("aligner_node_align_train", _inputs, _align_run, NODE, _state(True), upstream={"g"}, fixed={"x"}),
]
for _row in ROWS:                                                    # the table's own lists: its engine and its coverage test see these rows
    if _row.name not in table.BY_NAME:
        table.ROWS.append(_row)
        table.BY_NAME[_row.name] = _row

SINGLE = [(r.name, k, kind) for r in ROWS for k in r.inputs() for kind in r.kinds(k)]


@pytest.mark.parametrize("name,key,kind", SINGLE, ids=lambda v: str(v))
def test_one_input_in_another_layout(name, key, kind, gate):
    _check_case(table.BY_NAME[name], gate, {key: kind})


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_all_inputs_in_other_layouts_together(name, gate):
    row = table.BY_NAME[name]
    choice = {}
    for i, k in enumerate(row.inputs()):
        kinds = row.kinds(k)
        if kinds:
            choice[k] = kinds[i % len(kinds)]
    assert choice
    _check_case(row, gate, choice)


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_dense_case_on_a_side_stream(name, gate):
    row = table.BY_NAME[name]
    want = _reference(row)
    side, main = torch.cuda.Stream(device=DEV), torch.cuda.current_stream(DEV)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        got = row.run(row.state(), dict(_device_inputs(name)))
    main.wait_stream(side)
    torch.cuda.synchronize()
    for k in want:
        assert _bits_equal(got[k], want[k]), f"{name}: output {k} differs on a side stream"


def test_the_rows_reach_every_entry_of_the_trainable_form(gate):
    """What the table's coverage test needs of these rows, stated here too: with the weight images dropped, one dense run of the eval and
    the train row launches or asks every entry the trainable form adds to the package."""
    from e3dge_amd import _lib
    for name in ("aligner_node_eval", "aligner_node_train"):
        row = table.BY_NAME[name]
        _lib.invalidate(row.state())
        row.run(row.state(), dict(_device_inputs(name)))
    torch.cuda.synchronize()
    added = {"e3dge_aligner_saved_bytes", "e3dge_aligner_bwd_workspace_bytes", "e3dge_aligner_grad_offset", "e3dge_aligner_stats_channels",
             "e3dge_aligner_packed_t_floats", "e3dge_aligner_pack_t", "e3dge_aligner_forward_saving", "e3dge_aligner_backward",
             "e3dge_aligner_branch_count", "e3dge_aligner_branch_bytes"}
    assert added <= set(gate.names), added - set(gate.names)
