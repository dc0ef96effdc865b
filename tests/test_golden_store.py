"""oracle/golden_store.py: a re-recorded fixture over the size limit is written as a delta and read back bit for bit."""
import os

import numpy as np
import pytest

from oracle import golden_store


def test_over_the_limit_rerecording_round_trips_as_a_delta(tmp_path, monkeypatch):
    monkeypatch.setattr(golden_store, "MAX_BYTES", 20_000)
    rs = np.random.RandomState(0)
    first = {"x": rs.standard_normal(8192).astype(np.float32), "seed": np.int32(3), "f64": rs.standard_normal(64)}
    with pytest.raises(RuntimeError, match="no earlier recording"):
        golden_store.save(str(tmp_path), "fx", first)
    np.savez_compressed(tmp_path / "fx.npz", **first)
    second = {"x": np.nextafter(first["x"], np.float32(np.inf)), "seed": np.int32(3), "f64": -first["f64"],
              "new": np.arange(5.0)}
    path = golden_store.save(str(tmp_path), "fx", second)
    assert path.endswith("fx.delta.npz") and os.path.getsize(path) <= golden_store.MAX_BYTES
    got = golden_store.load(str(tmp_path), "fx")
    assert sorted(got.files) == sorted(second)
    for k, v in second.items():
        assert got[k].dtype == np.asarray(v).dtype and got[k].tobytes() == np.asarray(v).tobytes(), k
    small = {"x": np.zeros(4, np.float32)}
    assert golden_store.save(str(tmp_path), "fx", small).endswith("fx.npz") and not os.path.exists(path)
    assert golden_store.load(str(tmp_path), "fx")["x"].tobytes() == small["x"].tobytes()
