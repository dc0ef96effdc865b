"""CPU: the default library carries no cycle-stamp instrumentation (csrc/stamps.h) and says so: reading any unit's stamps raises
with the -D that an instrumented variant build needs, and the per-kernel debug exports of earlier builds are gone."""
import pytest

from e3dge_amd import _lib

SELECTORS = {"siren": ("-DE3DGE_PHASE_TIMING", "-DE3DGE_16_TRACE"), "siren_bwd": ("-DE3DGE_BWD_TIMING",), "resblock": ("-DE3DGE_RB_TRACE",),
             "modconv": ("-DE3DGE_MC_TIMING",), "decoder2": ("-DE3DGE_PK_TIMING",)}


def test_units_match_the_selectors():
    assert set(_lib.STAMP_UNITS) == set(SELECTORS)


@pytest.mark.parametrize("unit", _lib.STAMP_UNITS)
def test_default_library_is_not_instrumented(lib, unit):
    for call in (_lib.read_stamps, _lib.clear_stamps):
        with pytest.raises(RuntimeError) as e:
            call(unit)
        assert "not instrumented" in str(e.value)
        for define in SELECTORS[unit]:
            assert define in str(e.value)


def test_old_debug_exports_are_gone(lib):
    assert not hasattr(lib, "e3dge_debug_trace16")
    assert not hasattr(lib, "e3dge_debug_rb_trace")
