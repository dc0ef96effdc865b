"""GPU: the rows of the camera-pose predictor for the layouts table of tests/test_gpu_layouts.py -- forward() of
e3dge_amd.volume_discriminator.VolumeRenderDiscriminator and image2camsettings with the image in every layout of
tests/layout_variants.py and on a side stream; bit for bit the dense run's results, inputs untouched, no output in an input's buffer,
every pointer as the gate of that file wants it.

The rows are appended to that file's ROWS / BY_NAME when this file is imported, so that its engine (_check_case, the gate) runs them
and its coverage test (test_every_launched_entry_has_a_row_or_a_reason) drives the new entries through its own gate: the table is
extended from here because this file is new and that one is not.  Running that file without this one leaves the coverage test without
these rows."""
import pytest
import torch

import e3dge_amd  # noqa: F401
import test_gpu_layouts as table
from test_gpu_layouts import DEV, Row, _bits_equal, _check_case, _device_inputs, _reference, gate  # noqa: F401  (gate: autouse here too)

pytestmark = pytest.mark.gpu
FORWARD = {"e3dge_vdisc_forward"}


def _inputs16():
    from test_discriminator_host import golden_images
    return dict(x=golden_images(2, 16))


def _inputs64():
    from test_discriminator_host import golden_images
    return dict(x=golden_images(2, 64))


def _state(size):
    def build():
        from test_gpu_volume_disc import module_gpu
        return module_gpu(size, 'wide')
    return build


def _forward_run(m, t):
    with torch.no_grad():
        logits, views, taps = m.run(t["x"], taps=True)
    return dict(logits=logits, viewpoints=views, **{f"tap{i}": v for i, v in enumerate(taps)})


def _cam_run(m, t):
    from e3dge_amd.volume_discriminator import image2camsettings
    import test_volume_disc_host as host
    cam = image2camsettings(m, t["x"], host.CAMERA, 8, is_thumb=True)     # (the pooling has its own row, "avgpool", with its listed fallbacks)
    return {k: v for k, v in cam.items() if torch.is_tensor(v)}


ROWS = [
    Row("volume_disc_forward", _inputs16, _forward_run, FORWARD, _state(16)),
    Row("volume_disc_image2camsettings", _inputs64, _cam_run, FORWARD, _state(64)),
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


def test_the_rows_reach_every_entry_of_the_module(gate):
    """What the table's coverage test needs of these rows, stated here too: with the weight image dropped, one dense run launches or asks
    every entry the module adds to the package."""
    from e3dge_amd import _lib
    row = table.BY_NAME["volume_disc_forward"]
    _lib.invalidate(row.state())
    row.run(row.state(), dict(_device_inputs(row.name)))
    torch.cuda.synchronize()
    added = {"e3dge_vdisc_packed_floats", "e3dge_vdisc_pack_weights", "e3dge_vdisc_ws_bytes", "e3dge_vdisc_forward"}
    assert added <= set(gate.names), added - set(gate.names)
