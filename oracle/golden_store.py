"""How tests/golden/*.npz are stored.  TEST INFRASTRUCTURE.

A fixture is a set of named arrays.  No file under tests/golden/ may exceed MAX_BYTES.  When a fixture is recorded again and
comes to more than that, the earlier recording, <name>.npz, stays as it is and the new one is written beside it as
<name>.delta.npz: the list of keys, each floating-point array whose bits changed as the XOR of its bits with the earlier
recording's, split into byte planes (a re-recording moves mostly low bits, so the high planes are zeros and compress to
almost nothing), and every other changed or new array whole.  Arrays whose bits did not change are not stored again.
load() returns the new recording, bit for bit."""
import io
import os

import numpy as np

MAX_BYTES = 1_000_000
_KEYS = "__keys__"
_XOR = "xor__"


class Fixture(dict):
    """The arrays of a fixture; `.files` lists its keys like numpy's NpzFile."""

    @property
    def files(self):
        return list(self)


def _uint(a):
    return np.dtype(f"u{a.dtype.itemsize}")


def load(gold, name):
    base = np.load(os.path.join(gold, name + ".npz"))
    delta_path = os.path.join(gold, name + ".delta.npz")
    if not os.path.exists(delta_path):
        return base
    d = np.load(delta_path)
    out = Fixture()
    for k in map(str, d[_KEYS]):
        if _XOR + k in d.files:
            b = base[k]
            x = np.ascontiguousarray(d[_XOR + k].T).view(_uint(b)).reshape(b.shape)
            out[k] = (b.view(_uint(b)) ^ x).view(b.dtype)
        else:
            out[k] = d[k] if k in d.files else base[k]
    return out


def _npz_bytes(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def save(gold, name, arrays):
    """Write a recording of fixture `name`; returns the path written."""
    path, delta_path = (os.path.join(gold, name + ext) for ext in (".npz", ".delta.npz"))
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    data = _npz_bytes(arrays)
    if len(data) > MAX_BYTES:
        if not os.path.exists(path):
            raise RuntimeError(f"{name}: {len(data)} bytes is over {MAX_BYTES} and there is no earlier recording to store it against")
        base = np.load(path)
        out = {_KEYS: np.array(list(arrays))}
        for k, v in arrays.items():
            b = base[k] if k in base.files else None
            if b is not None and b.dtype == v.dtype and b.shape == v.shape:
                bits = v.view(_uint(v)) ^ b.view(_uint(b)) if v.dtype.kind == "f" else None
                if (bits is not None and not bits.any()) or (bits is None and np.array_equal(v, b)):
                    continue
                if bits is not None:
                    out[_XOR + k] = np.ascontiguousarray(bits.reshape(-1).view(np.uint8).reshape(-1, v.dtype.itemsize).T)
                    continue
            out[k] = v
        data = _npz_bytes(out)
        if len(data) > MAX_BYTES:
            raise RuntimeError(f"{name}: the delta against the earlier recording is {len(data)} bytes, over {MAX_BYTES}")
        path, stale = delta_path, None
    else:
        stale = delta_path
    with open(path, "wb") as f:
        f.write(data)
    if stale and os.path.exists(stale):
        os.remove(stale)
    return path
