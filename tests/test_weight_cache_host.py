"""Host side of the weight-image cache (_lib.cached / latest / invalidate): CPU tensors and build functions that count their calls.
What every packed weight image, style table and plan of the package goes through: a hit needs the same source tensor OBJECTS (held by
the entry) with unchanged data pointer and version and an equal extra key; entries live in one module-level weak map."""
import copy
import gc
import weakref

import pytest
import torch
from torch import nn

import e3dge_amd  # noqa: F401
from e3dge_amd import _lib
from e3dge_amd import synthetic as syn


class Leaf(nn.Module):
    def __init__(self, n=4):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(n))


class Top(nn.Module):
    """The cached module sits two levels below the top."""

    def __init__(self):
        super().__init__()
        self.mid = nn.Sequential(Leaf())

    @property
    def leaf(self):
        return self.mid[0]


class Image:
    """`Image(mod)()`: the cached copy of mod.weight, and how often it was built."""

    def __init__(self, mod, slot='image', limit=1):
        self.mod, self.slot, self.limit, self.builds = mod, slot, limit, 0

    def _build(self):
        self.builds += 1
        return self.mod.weight.detach().clone()

    def __call__(self, extra=()):
        return _lib.cached(self.mod, self.slot, (self.mod.weight,), self._build, extra, self.limit)


def test_hit_after_no_change_and_rebuild_after_every_visible_change():
    m = Leaf()
    img = Image(m)
    a = img()
    assert img() is a and img.builds == 1                                  # no change: a hit
    m.train(), m.eval(), m.float()                                         # (train() / a no-op _apply change nothing: still a hit)
    assert img() is a and img.builds == 1
    with torch.no_grad():
        m.weight.add_(1)                                                   # in-place op: version
    assert float(img()[0]) == 1 and img.builds == 2
    m.load_state_dict({'weight': torch.full((4,), 3.0)})                   # load_state_dict copies in place: version
    assert float(img()[0]) == 3 and img.builds == 3
    m.weight.data = torch.full((4,), 5.0)                                  # p.data = other: pointer (the version stays)
    assert float(img()[0]) == 5 and img.builds == 4
    m.double()                                                             # what .to() does: _apply swaps .data under the same Parameter
    assert img().dtype == torch.float64 and img.builds == 5
    assert img() is img() and img.builds == 5
    b = img(extra=('cuda:1',))                                             # the extra key (device, batch, resolution, stream)
    assert img.builds == 6 and img(extra=('cuda:1',)) is b


def test_replaced_parameter_at_the_same_address_and_version_is_rebuilt():
    """A (data_ptr, _version) key cannot tell a Parameter from its replacement on the same storage (what the caching allocator hands
    out after a free); the entry holds the tensor it was built from and compares identity."""
    buf = torch.zeros(4)
    m = Leaf()
    m.weight = p1 = nn.Parameter(buf)
    img = Image(m)
    assert float(img()[0]) == 0
    p1.data.fill_(2)
    m.weight = p2 = nn.Parameter(buf)
    assert p2 is not p1 and (p2.data_ptr(), p2._version) == (p1.data_ptr(), p1._version)
    assert float(img()[0]) == 2 and img.builds == 2


def test_data_write_is_stale_until_invalidate_on_the_parent():
    top = Top()
    img = Image(top.leaf)
    img()
    top.leaf.weight.data.fill_(7)                                          # bumps no version
    assert float(img()[0]) == 0 and img.builds == 1                        # served stale, as documented
    _lib.invalidate(top)                                                   # two levels above the module that owns the entry
    assert float(img()[0]) == 7 and img.builds == 2


@pytest.mark.parametrize("kind", ["single", "slots", "dependent"])
def test_strict_mode_sees_data_writes_at_every_kind_of_site(kind, monkeypatch):
    monkeypatch.setattr(_lib, "STRICT_WEIGHT_CACHE", True)
    top = Top()
    m = top.leaf
    src = Image(m, 'src')
    if kind == "single":
        get = Image(m)
    elif kind == "slots":
        table = Image(m, 'table', limit=8)
        get = lambda: table(extra=(2, 'cpu', 0))
    else:
        n = [0]

        def get():
            s = src()
            return _lib.cached(top, 'plan', [m.weight, s], lambda: (n.__setitem__(0, n[0] + 1), s.clone())[1])
    a = get()
    assert get() is a
    m.weight.data.fill_(4)
    b = get()
    assert b is not a and float(b[0]) == 4
    assert get() is b


def test_deepcopy_state_dict_and_pickling_never_see_a_cache():
    top = Top()
    img = Image(top.leaf)
    keys, attrs = list(top.state_dict()), {k: set(vars(v)) for k, v in top.named_modules()}
    a = img()
    assert list(top.state_dict()) == keys
    assert {k: set(vars(v)) for k, v in top.named_modules()} == attrs      # no cache attribute on any module
    twin = copy.deepcopy(top)
    assert twin.leaf not in _lib._WEIGHT_CACHE and _lib.latest(twin.leaf, 'image') is None
    img2 = Image(twin.leaf)
    assert img2() is not a and img2.builds == 1 and img() is a


def test_entries_die_with_their_module():
    gc.collect()
    before = len(_lib._WEIGHT_CACHE)
    top = Top()
    Image(top.leaf)()
    ref = weakref.ref(top.leaf)
    assert len(_lib._WEIGHT_CACHE) == before + 1
    del top
    gc.collect()
    assert ref() is None and len(_lib._WEIGHT_CACHE) == before


def test_slot_eviction_drops_the_oldest_only():
    m = Leaf()
    N = 4
    tab = Image(m, 'table', limit=N)
    vals = [tab(extra=(b, 'cpu', 0)) for b in range(N)]
    assert tab.builds == N and all(tab(extra=(b, 'cpu', 0)) is v for b, v in enumerate(vals))
    extra_one = tab(extra=(N, 'cpu', 0))                                   # entry N + 1
    assert tab.builds == N + 1
    assert all(tab(extra=(b, 'cpu', 0)) is vals[b] for b in range(1, N)) and tab(extra=(N, 'cpu', 0)) is extra_one
    assert tab.builds == N + 1                                             # the others still hit
    assert tab(extra=(0, 'cpu', 0)) is not vals[0] and tab.builds == N + 2   # only the oldest went


def test_dependent_entry_follows_its_source_even_at_the_old_address():
    """The style table is built from the squared-norm tables, the plan from the table: when a source value is rebuilt, what was derived
    from it is rebuilt too -- also when the new value lands where the old one was (shared storage stands in for the allocator)."""
    top = Top()
    store = torch.zeros(4)
    n = {'src': 0, 'plan': 0}

    def source():
        def build():
            n['src'] += 1
            return store[:]                                                # a new tensor object on the same storage, same version
        return _lib.cached(top.leaf, 'wsq', (top.leaf.weight,), build)

    def plan():
        s = source()

        def build():
            n['plan'] += 1
            return float(s[0])
        return _lib.cached(top, 'plan', (top.leaf.weight, s), build)
    assert plan() == 0 and plan() == 0 and n == {'src': 1, 'plan': 1}
    old = source()
    store.data.fill_(3)
    _lib.invalidate(top.leaf)                                              # the source's entry only
    new = source()
    assert new is not old and (new.data_ptr(), new._version) == (old.data_ptr(), old._version)
    assert plan() == 3 and n == {'src': 2, 'plan': 2}


def _generator():
    from e3dge_amd.stylesdf_model import G_pred_latents
    g = G_pred_latents(syn.model_opt(size=64, channel_multiplier=1, renderer_spatial_output_dim=16), syn.rendering_opt(N_samples=6),
                       full_pipeline=True)
    syn.load_synthetic(g)
    return g.eval()


def test_the_real_host_side_sites_follow_the_same_rules(monkeypatch):
    """sigmoid_beta's host copy and the decoder's blur factor are the two sites that work without a GPU."""
    from e3dge_amd.stylesdf_model import blur_factor, make_kernel
    g = _generator()
    keys, attrs = list(g.state_dict()), {k: set(vars(v)) for k, v in g.named_modules()}
    r, dec = g.renderer, g.decoder
    sb = r._sigmoid_beta_value()
    bf = dec._blur_factor()
    assert bf == blur_factor(dec.convs[0].conv.blur.kernel) and bf is dec._blur_factor()
    assert list(g.state_dict()) == keys and {k: set(vars(v)) for k, v in g.named_modules()} == attrs
    for m in g.modules():                                                  # every module that caches can be told to forget
        if type(m).__name__ in ("SirenGenerator", "ResnetBlockFC", "ModulatedConv2d", "VolumeFeatureRenderer", "Decoder", "Generator"):
            assert callable(m.invalidate)
    r.sigmoid_beta.data.mul_(2)
    dec.convs[0].conv.blur.kernel.data.copy_(make_kernel([1, 2, 2, 1]) * 4)
    assert r._sigmoid_beta_value() == sb and dec._blur_factor() is bf      # stale, as documented
    g.invalidate()                                                         # reaches the renderer and the decoder
    assert r._sigmoid_beta_value() == pytest.approx(2 * sb) and dec._blur_factor() != bf
    twin = copy.deepcopy(g)                                                # (the reference builds its EMA copy this way)
    assert all(m not in _lib._WEIGHT_CACHE for m in twin.modules())
    monkeypatch.setattr(_lib, "STRICT_WEIGHT_CACHE", True)
    g.invalidate()
    sb = r._sigmoid_beta_value()
    r.sigmoid_beta.data.mul_(-1)                                           # (same norm: the fingerprint is more than a norm)
    assert r._sigmoid_beta_value() == pytest.approx(-sb)


def test_fuse_sft_mlp_has_invalidate():
    from e3dge_amd.local_query import Fuse_sft_MLP
    m = Fuse_sft_MLP(257, 256)
    keys = list(m.state_dict())
    m.invalidate()
    assert list(m.state_dict()) == keys
