"""Host time of one weight-cache hit, without a GPU: the lookup every launch wrapper makes (_lib.cached over the module's parameters)
beside the comparison it replaced (a tuple of (data_ptr, _version) per parameter against the stored one), for the SIREN's parameter
set and for one ModulatedConv2d.   python tools/weight_cache_host_time.py"""
import os
import sys
import timeit

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import e3dge_amd  # noqa: F401,E402
from e3dge_amd import _lib  # noqa: E402
from e3dge_amd.stylesdf_model import ModulatedConv2d  # noqa: E402
from e3dge_amd.volume_renderer import SirenGenerator  # noqa: E402


def us(fn, n=20000):
    return 1e6 * min(timeit.repeat(fn, number=n, repeat=7)) / n


siren = SirenGenerator()
ps = _lib.params_of(siren)
old_key = tuple((q.data_ptr(), q._version) for q in ps)
image = object()
old = us(lambda: tuple((q.data_ptr(), q._version) for q in _lib.params_of(siren)) == old_key)
new = us(lambda: _lib.cached(siren, 'image', _lib.params_of(siren), lambda: image))
print(f"SirenGenerator ({len(ps)} tensors): (data_ptr, _version) tuple compare {old:.2f} us, _lib.cached hit {new:.2f} us")

conv = ModulatedConv2d(256, 256, 3, 512)
w = conv.weight
conv_key = (w.data_ptr(), w._version, str(w.device))
conv._probe, conv._probe_key = image, conv_key


def old_conv():
    w = conv.weight
    key = (w.data_ptr(), w._version, str(w.device))
    return getattr(conv, '_probe', None) is None or conv._probe_key != key


old = us(old_conv)
new = us(lambda: _lib.cached(conv, 'image', (conv.weight,), lambda: image))
print(f"ModulatedConv2d (1 tensor): attribute key compare {old:.2f} us, _lib.cached hit {new:.2f} us")
