"""CPU: the inputs of tests/test_gpu_fir_parity.py are fit to find a wrong tap -- and the parts of the FIR code that need no GPU.

Every 4x4 FIR the older GPU tests feed to a tiled kernel equals its own 180-degree flip, so a dropped flip, a transposed tap index or
swapped pads changes nothing they look at.  This file fixes ONE asymmetric 4x4 FIR (asym_fir: seeded, mixed signs, not rank one,
invariant under no flip and not under transposition, sum|k| = 1) and the geometries of the GPU file (GEOMETRIES: the tiled kernels at
the smallest sizes with more than one tile and a ragged last tile per axis; GENERIC: the one-output-per-thread kernel) and shows, in
float64 on the oracle alone:

  sensitivity   for every geometry, the oracle differs from itself by more than 1000 x the GPU file's bound when the FIR is left
                unflipped, when it is transposed, when pad0 / pad1 are swapped and when the input is shifted by one pixel in x or y.
                A mutation that is the identity for a geometry (pad0 == pad1; a 1 x 1 FIR's flip; a non-square FIR cannot be
                transposed in place) is no mistake a kernel could make there and is not asked for; the test asserts which ones apply.
  CPU branch    op.upfirdn2d on CPU tensors equals the oracle in float64 with difference 0.
  adjoint       Geometry.adjoint with the flipped FIR is the transposed operator: <A x, y> = <x, A^T y> to 1e-12 relative in float64,
                A^T evaluated through _upfirdn2d_cpu (no autograd).
  image metrics the float64 per-pixel reference of tests/test_gpu_metrics.py's per-tile tests (metrics_pixels_ref) against
                sharded_eval.image_metrics_torch in float64: the eight columns to 1e-12.
  decoder oracle  oracle/decoder_ref's optional FIR arguments: the defaults give the bits they gave before the arguments existed.
  decoder         Decoder._blur_factor (what _dec2_ok asks before it takes the packed pipeline, which hands level 0's kernels to every
                  level) is None as soon as one level's Blur or Upsample buffer differs from level 0's.

Bound (the project's standing one, parity_bound of tests/test_encoder_host.py): per tensor max|hip - f64| <= max(2e-6 max|f64|,
3 max|f32 - f64|), f32 the same CPU composition in float32."""
import functools
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import decoder_ref, ops_ref

import e3dge_amd  # noqa: F401
from e3dge_amd import sharded_eval as se

up_mod = importlib.import_module("e3dge_amd.op.upfirdn2d")          # (the package's attribute of that name is the function)
Geometry = up_mod.Geometry

from test_encoder_host import parity_bound

FIR_SEED = 3
SENSITIVITY = 1000.0


@functools.lru_cache(maxsize=None)
def asym_fir(gain=1.0):
    """The one asymmetric 4x4 FIR of the FIR tests, float64: N(0, 1) taps of a seeded generator, sum|k| = gain (4 for the up-by-2
    cases, as Upsample scales its kernel by factor^2)."""
    k = torch.randn(4, 4, generator=torch.Generator().manual_seed(FIR_SEED), dtype=torch.float64)
    return k / k.abs().sum() * gain


class Geo:
    """One case: kind 'blur' / 'up' / 'down' (the tiled kernels, square up / down, scalar pads as the public op takes them) or
    'generic' (up, down per axis (x, y), pad (x0, x1, y0, y1), any FIR)."""

    def __init__(self, name, kind, in_hw, pad, out_hw, up=1, down=1, fir=None, planes=(2, 2), grads=True):
        self.name, self.kind, self.in_hw, self.out_hw, self.planes, self.grads = name, kind, in_hw, out_hw, planes, grads
        sq = lambda v: (v, v) if isinstance(v, int) else tuple(v)
        self.up, self.down = sq(up), sq(down)
        self.pad = tuple(pad) if len(pad) == 4 else (pad[0], pad[1], pad[0], pad[1])
        self.square = isinstance(up, int) and isinstance(down, int) and len(pad) == 2
        self._fir = fir
        self.tile = {"blur": (64, 64), "up": (32, 64), "down": (32, 64)}.get(kind)

    @property
    def fir(self):
        return self._fir if self._fir is not None else asym_fir(4.0 if self.kind == "up" else 1.0)

    @property
    def geometry(self):
        return Geometry(self.up, self.down, self.pad)

    def x(self, dtype=torch.float64):
        """N(0, 1) planes (B, C, H, W), seeded by the case's name; float32 values, so that every dtype sees the same numbers."""
        g = torch.Generator().manual_seed(sum(ord(c) * (i + 1) for i, c in enumerate(self.name)))
        return torch.randn(*self.planes, *self.in_hw, generator=g, dtype=torch.float32).to(dtype)

    def gy(self, dtype=torch.float64):
        g = torch.Generator().manual_seed(7 + sum(ord(c) * (i + 1) for i, c in enumerate(self.name)))
        return torch.randn(*self.planes, *self.out_hw, generator=g, dtype=torch.float32).to(dtype)

    def ref(self, x, fir=None, pad=None):
        return ops_ref.upfirdn2d_ref(x, (self.fir if fir is None else fir).to(x.dtype), self.up, self.down, self.pad if pad is None else pad)

    def __repr__(self):
        return self.name


def _generic_fir(kh, kw, seed):
    k = torch.randn(kh, kw, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return k / k.abs().sum()


GEOMETRIES = [
    # Blur, up 1 / down 1: blur44_kernel, 64 x 64 output tiles
    Geo("blur_70x131", "blur", (70, 131), (2, 1), (70, 131)),        # W % 4 = 3, 2 x 3 tiles
    Geo("blur_65x69", "blur", (65, 69), (1, 1), (64, 68)),           # float4 stores, a 4-wide last tile
    Geo("blur_17x17", "blur", (17, 17), (2, 2), (18, 18)),           # the discriminator's pad
    Geo("blur_70x70_crop", "blur", (70, 70), (-1, 0), (66, 66)),     # crop
    Geo("blur_4x4", "blur", (4, 4), (0, 0), (1, 1)),                 # smallest case
    # Upsample, up 2: upfirdn2d_tiled_kernel<2, 1, 4, 4>, 32 x 64 output tiles
    Geo("up_35x67", "up", (35, 67), (2, 1), (70, 134), up=2),        # W % 4 = 2, 3 x 3 tiles
    Geo("up_17x34", "up", (17, 34), (2, 1), (34, 68), up=2),         # vector stores
    Geo("up_19x23_crop", "up", (19, 23), (-1, 2), (36, 44), up=2),   # the existing crop
    Geo("up_1x1", "up", (1, 1), (2, 1), (2, 2), up=2),               # smallest case
    # Downsample, down 2: upfirdn2d_tiled_kernel<1, 2, 4, 4>
    Geo("down_67x133", "down", (67, 133), (1, 1), (33, 66), down=2),     # ragged tiles
    Geo("down_130x262", "down", (130, 262), (2, 2), (66, 132), down=2),  # vector stores, 3 x 3 tiles
    Geo("down_5x5", "down", (5, 5), (1, 1), (2, 2), down=2),             # smallest case
]
GENERIC = [
    # the geometry of the `asym` fixture of tests/golden/upfirdn2d.npz (3 x 5 taps, every parameter different per axis)
    Geo("gen_asym3x5", "generic", (10, 14), (1, 2, 0, 3), (4, 27), up=(2, 1), down=(1, 3), fir=_generic_fir(3, 5, 11)),
    Geo("gen_5x5_up3_down2", "generic", (9, 14), (3, 2), (14, 22), up=3, down=2, fir=_generic_fir(5, 5, 12)),
    Geo("gen_1x1", "generic", (6, 9), (1, 2), (9, 12), fir=_generic_fir(1, 1, 13)),
    Geo("gen_4x4_up2x1", "generic", (12, 21), (2, 1, 2, 1), (12, 42), up=(2, 1)),     # up not square: no tiled kernel
    # more than 16384 x 256 outputs: the grid-stride loop of the generic kernel runs more than once
    Geo("gen_stride_loop", "generic", (1000, 900), (1, 1), (1000, 900), fir=_generic_fir(3, 3, 14), planes=(1, 5), grads=False),
]
ALL = GEOMETRIES + GENERIC


def test_the_geometries_are_what_their_names_say():
    for c in ALL:
        kh, kw = c.fir.shape
        assert c.geometry.out_hw(c.in_hw[0], c.in_hw[1], kh, kw) == c.out_hw, c
    tiled = {c.name: c for c in GEOMETRIES}
    assert all(tuple(c.fir.shape) == (4, 4) and c.square for c in GEOMETRIES)
    # more than one tile and a ragged last tile on each axis, for each tiled kernel
    for n in ("blur_70x131", "up_35x67", "down_67x133", "down_130x262"):
        c = tiled[n]
        assert all(o > t and o % t for o, t in zip(c.out_hw, c.tile)), n
    assert tiled["blur_70x131"].out_hw[1] % 4 == 3 and tiled["up_35x67"].out_hw[1] % 4 == 2
    assert all(tiled[n].out_hw[1] % 4 == 0 for n in ("blur_65x69", "up_17x34", "down_130x262", "up_19x23_crop"))
    assert tiled["blur_65x69"].out_hw[1] - 64 == 4
    big = GENERIC[-1]
    assert big.planes[0] * big.planes[1] * big.out_hw[0] * big.out_hw[1] > 16384 * 256
    assert GENERIC[3].up[0] != GENERIC[3].up[1] and tuple(GENERIC[3].fir.shape) == (4, 4)
    golden_cfg = (2, 1, 1, 3, 1, 2, 0, 3)                            # ux, uy, dx, dy, px0, px1, py0, py1 of the `asym` fixture
    assert GENERIC[0].up + GENERIC[0].down + GENERIC[0].pad == golden_cfg and GENERIC[0].in_hw == (10, 14)


def test_the_fir_has_no_symmetry_a_kernel_could_hide_behind():
    k = asym_fir()
    m = float(k.abs().max())
    assert abs(float(k.abs().sum()) - 1.0) <= 1e-15 and abs(float(asym_fir(4.0).abs().sum()) - 4.0) <= 1e-14
    for name, other in (("flip", k.flip(0, 1)), ("transpose", k.t()), ("flip_y", k.flip(0)), ("flip_x", k.flip(1)),
                        ("flip_transpose", k.flip(0, 1).t())):
        assert float((k - other).abs().max()) >= 0.5 * m, name
    assert float(k.min()) <= -0.5 * m and float(k.max()) >= 0.5 * m             # mixed signs
    s = torch.linalg.svdvals(k)
    assert float(s[1] / s[0]) >= 0.25                                            # not rank one: no pair of 1-D passes applies it
    assert abs(float(k.sum())) >= 0.1 * float(k.abs().sum())                     # a constant plane is not annihilated
    # the inner 2 x 2 block (all that a 1 x 1 plane up-sampled by 2 ever meets) is asymmetric too
    c = k[1:3, 1:3]
    assert float((c - c.flip(0, 1)).abs().max()) >= 0.1 * m and float((c - c.t()).abs().max()) >= 0.1 * m


def _shift(x, dy, dx):
    """x moved by (dy, dx) pixels, zeros moved in."""
    out = torch.zeros_like(x)
    H, W = x.shape[2:]
    out[:, :, dy:, dx:] = x[:, :, :H - dy, :W - dx]
    return out


def mutations(c):
    """{name: float64 result of the mutated oracle} for every mutation that is not the identity for this geometry."""
    x = c.x()
    k = c.fir
    out = {}
    if not torch.equal(k, k.flip(0, 1)):
        out["unflipped"] = c.ref(x, fir=k.flip(0, 1))
    if k.shape[0] == k.shape[1] and not torch.equal(k, k.t()):
        out["transposed"] = c.ref(x, fir=k.t())
    px0, px1, py0, py1 = c.pad
    if (px0, py0) != (px1, py1):
        out["pads_swapped"] = c.ref(x, pad=(px1, px0, py1, py0))
    out["shift_x"] = c.ref(_shift(x, 0, 1))
    out["shift_y"] = c.ref(_shift(x, 1, 0))
    return out


@pytest.mark.parametrize("c", ALL, ids=repr)
def test_every_mutation_moves_the_oracle_by_a_thousand_bounds(c):
    x = c.x()
    y64, y32 = c.ref(x), c.ref(x.float())
    bound = parity_bound(y64, y32)
    muts = mutations(c)
    want = {"shift_x", "shift_y"}
    if c.fir.numel() > 1:
        want.add("unflipped")
        if c.fir.shape[0] == c.fir.shape[1]:
            want.add("transposed")
    if c.pad[0] != c.pad[1] or c.pad[2] != c.pad[3]:
        want.add("pads_swapped")
    assert set(muts) == want, (c, sorted(muts))
    assert bound <= 3e-6 * float(y64.abs().max())                    # the float32 oracle is a yardstick: a few 1e-7 of the maximum
    for name, ym in muts.items():
        assert ym.shape == y64.shape
        d = float((ym - y64).abs().max())
        assert d >= SENSITIVITY * bound, (c, name, d, bound)


@pytest.mark.parametrize("c", ALL, ids=repr)
def test_cpu_branch_is_the_oracle(c):
    x, k = c.x(), c.fir
    want = c.ref(x)
    got = up_mod._upfirdn2d_cpu(x, k, c.geometry)
    assert got.dtype == torch.float64 and got.shape == want.shape and float((got - want).abs().max()) == 0.0
    if c.square:
        pub = up_mod.upfirdn2d(x, k, up=c.up[0], down=c.down[0], pad=(c.pad[0], c.pad[1]))
        assert float((pub - want).abs().max()) == 0.0


@pytest.mark.parametrize("c", ALL, ids=repr)
def test_adjoint_geometry_with_the_flipped_fir_is_the_transpose(c):
    x, y, k = c.x(), c.gy(), c.fir
    kh, kw = k.shape
    ax = up_mod._upfirdn2d_cpu(x, k, c.geometry)
    adj = c.geometry.adjoint(c.in_hw[0], c.in_hw[1], kh, kw)
    aty = up_mod._upfirdn2d_cpu(y, torch.flip(k, [0, 1]), adj)
    assert tuple(aty.shape) == tuple(x.shape)
    lhs, rhs = float((ax * y).sum()), float((x * aty).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (c, lhs, rhs)
    # and the adjoint of the adjoint is the operator itself
    back = adj.adjoint(c.out_hw[0], c.out_hw[1], kh, kw)
    assert float((up_mod._upfirdn2d_cpu(x, k, back) - ax).abs().max()) == 0.0


# ---- image metrics: the per-pixel reference of the per-tile GPU tests ---------------------------------------------------------------
def metrics_pixels_ref(pred, gt):
    """(squared error, absolute error, SSIM loss) per pixel, each (B, C, H, W), in the dtype of the inputs: 5-tap Gaussian window with
    sigma 1.5, reflect padding by 2, C1 = 0.01^2, C2 = 0.03^2, loss = clamp((1 - ssim) / 2, 0, 1) -- written out tap by tap, not
    through conv2d: the window is a plain sum over 25 shifted views."""
    dt = pred.dtype
    t = torch.arange(5, dtype=dt) - 2
    g = torch.exp(-(t * t) / (2 * 1.5 * 1.5))
    g = g / g.sum()
    H, W = pred.shape[2:]

    def win(v):
        p = F.pad(v, [2, 2, 2, 2], mode="reflect")
        acc = torch.zeros_like(v)
        for i in range(5):
            for j in range(5):
                acc = acc + (g[i] * g[j]) * p[:, :, i:i + H, j:j + W]
        return acc
    mx, my = win(pred), win(gt)
    sxx, syy, sxy = win(pred * pred) - mx * mx, win(gt * gt) - my * my, win(pred * gt) - mx * my
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    ssim = ((2 * mx * my + c1) * (2 * sxy + c2)) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    d = pred - gt
    return d * d, d.abs(), torch.clamp((1 - ssim) / 2, 0, 1)


def metrics_tile_rows(pixels, tile=32):
    """(B * C * tiles_y * tiles_x, 3): the three per-pixel maps summed over each tile x tile block of each plane, in the order the kernel
    numbers its workgroups (plane, tile row, tile column)."""
    cols = []
    for m in pixels:
        B, C, H, W = m.shape
        ty, tx = -(-H // tile), -(-W // tile)
        p = F.pad(m, [0, tx * tile - W, 0, ty * tile - H])
        cols.append(p.reshape(B * C, ty, tile, tx, tile).sum((2, 4)).reshape(-1))
    return torch.stack(cols, 1)


METRIC_SHAPES = [(2, 3, 33, 65), (1, 2, 32, 32), (1, 3, 64, 96), (1, 1, 3, 3), (1, 1, 5, 33)]
EQUAL_TILE = {(1, 3, 64, 96): (1, 1, 1)}            # shape -> (plane, tile row, tile column) whose pixels (and halo) have pred == gt


def metrics_inputs(shape):
    """(pred, gt) float32 in (-1, 1): tanh of a smooth field plus noise, different per plane and not symmetric under transposition.  For
    the shape of EQUAL_TILE, pred == gt bit for bit on one tile and the two pixels around it that its windows reach."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(100 * H + W)
    yy = torch.linspace(-1, 1, H, dtype=torch.float64).reshape(1, 1, H, 1)
    xx = torch.linspace(-1, 1, W, dtype=torch.float64).reshape(1, 1, 1, W)
    ph = torch.rand(B, C, 1, 1, generator=g, dtype=torch.float64) * 6.28
    fr = 1 + 4 * torch.rand(B, C, 1, 1, generator=g, dtype=torch.float64)
    smooth = torch.sin(fr * xx + ph) * torch.cos(0.5 * fr * yy - ph) + 0.3 * xx - 0.2 * yy * xx
    gt = torch.tanh(smooth + 0.3 * torch.randn(shape, generator=g, dtype=torch.float64)).float()
    pred = torch.tanh(1.2 * gt.double() + 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)).float()
    if shape in EQUAL_TILE:
        p, ty, tx = EQUAL_TILE[shape]
        r0, r1, c0, c1 = max(32 * ty - 2, 0), min(32 * ty + 34, H), max(32 * tx - 2, 0), min(32 * tx + 34, W)
        pred = pred.clone()
        pred.view(B * C, H, W)[p, r0:r1, c0:c1] = gt.view(B * C, H, W)[p, r0:r1, c0:c1]
    return pred, gt


@pytest.mark.parametrize("shape", METRIC_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_metrics_pixel_reference_is_image_metrics_torch(shape):
    pred, gt = metrics_inputs(shape)
    B, C, H, W = shape
    for plane_p, plane_g in zip(pred.reshape(B * C, H, W), gt.reshape(B * C, H, W)):
        if H == W:
            assert not torch.equal(plane_p, plane_p.t()) and not torch.equal(plane_g, plane_g.t())
    assert len({t.numpy().tobytes() for t in pred.reshape(B * C, -1)}) == B * C          # planes differ
    p64, g64 = pred.double(), gt.double()
    se_, ae, sl = metrics_pixels_ref(p64, g64)
    want = se.image_metrics_torch(p64, g64)
    mse = se_.mean()
    mine = torch.stack([mse, mse * 0, mse * 0, mse, ae.mean(), 10 * torch.log10(1 / (mse / 4)), 1 - sl.mean(), mse * 0 + 1])
    assert mine.shape == want.shape == (8,)
    assert float((mine - want).abs().max()) <= 1e-12, (mine, want)
    rows = metrics_tile_rows((se_, ae, sl))
    assert rows.shape == (B * C * math.ceil(H / 32) * math.ceil(W / 32), 3)
    assert float((rows.sum(0) - torch.stack([se_.sum(), ae.sum(), sl.sum()])).abs().max()) <= 1e-9
    if shape in EQUAL_TILE:
        p, ty, tx = EQUAL_TILE[shape]
        row = rows[(p * math.ceil(H / 32) + ty) * math.ceil(W / 32) + tx]
        assert float(row.abs().max()) == 0.0 and int((rows.abs().sum(1) == 0).sum()) == 1


# ---- oracle/decoder_ref: the optional FIR arguments ----------------------------------------------------------------------------------
def _decoder_case():
    from e3dge_amd import synthetic as syn
    from conftest import full_state_dict
    g, sd = full_state_dict(size=32, cm=1, res=8)
    feats, noises, _ = syn.decoder_grad_inputs(1, 32, 8, seed=5)
    wd = torch.randn(1, g.decoder.n_latent, 512, generator=torch.Generator().manual_seed(5))
    return sd, feats, wd, noises


def test_decoder_oracle_defaults_are_unchanged_by_the_fir_arguments():
    """The default FIR is make_kernel([1, 3, 3, 1]) * 4: passing it explicitly, per stage or per level, gives the same bits as passing
    nothing, in float32 and float64; an asymmetric one moves the image."""
    sd, feats, wd, noises = _decoder_case()
    k = decoder_ref.fir(gain=4.0, dtype=torch.float64)
    for dt in (torch.float32, torch.float64):
        ref = decoder_ref.decoder_forward(sd, feats, wd, noises=noises, dtype=dt)
        same = decoder_ref.decoder_forward(sd, feats, wd, noises=noises, dtype=dt, blur_firs=[k, k], up_firs=[k, k])
        assert torch.equal(ref, same)
        stages = decoder_ref.decoder_stages(sd)
        x = decoder_ref.decoder_stage(sd, stages[0], feats, wd[:, 0], noises[0], dtype=dt)
        a = decoder_ref.decoder_stage(sd, stages[2], x, wd[:, 1], noises[1], dtype=dt)
        b = decoder_ref.decoder_stage(sd, stages[2], x, wd[:, 1], noises[1], dtype=dt, fir=k)
        assert torch.equal(a, b)
        assert torch.equal(decoder_ref.modulated_conv(sd, 'decoder.convs.0.conv.', x, wd[:, 1].to(dt), upsample=True),
                           decoder_ref.modulated_conv(sd, 'decoder.convs.0.conv.', x, wd[:, 1].to(dt), upsample=True, blur_fir=k))
        skip = decoder_ref.to_rgb(sd, 'decoder.to_rgb1.', x, wd[:, 1].to(dt), None, upsample=False)
        assert torch.equal(decoder_ref.to_rgb(sd, 'decoder.to_rgbs.0.', a, wd[:, 3].to(dt), skip),
                           decoder_ref.to_rgb(sd, 'decoder.to_rgbs.0.', a, wd[:, 3].to(dt), skip, up_fir=k))
    moved = decoder_ref.decoder_forward(sd, feats, wd, noises=noises, dtype=torch.float64, up_firs=[asym_fir(4.0)] * 2)
    assert float((moved - ref).abs().max()) > 1e-3


def test_decoder_with_per_level_fir_buffers_has_no_blur_factor():
    """No GPU needed: the cached answer follows in-place writes to any level's buffer, and comes back with the buffer."""
    import copy
    from conftest import full_state_dict
    from e3dge_amd import stylesdf_model as sm
    g, _ = full_state_dict(size=32, cm=1, res=8)
    dec = copy.deepcopy(g.decoder)
    assert len(dec.to_rgbs) == 2 and dec._blur_factor() == (0.25, 0.75, 0.75, 0.25)
    k0_blur, k0_up = dec.convs[0].conv.blur.kernel.clone(), dec.to_rgbs[0].upsample.kernel.clone()
    other = sm.make_kernel([1, 2, 2, 1]) * 4
    assert sm.blur_factor(other) is not None                          # on its own as good a blur as level 0's
    for buf, back in ((dec.convs[2].conv.blur.kernel, k0_blur), (dec.to_rgbs[1].upsample.kernel, k0_up)):
        with torch.no_grad():
            buf.copy_(other)
        assert dec._blur_factor() is None
        with torch.no_grad():
            buf.copy_(back)
        assert dec._blur_factor() == (0.25, 0.75, 0.75, 0.25)
    with torch.no_grad():                                             # the same asymmetric up-sampling kernel at EVERY level stays packed
        for tr in dec.to_rgbs:
            tr.upsample.kernel.copy_(asym_fir(4.0))
    assert dec._blur_factor() == (0.25, 0.75, 0.75, 0.25)
    with torch.no_grad():                                             # an asymmetric blur at every level: planar, as before
        for u in range(2):
            dec.convs[2 * u].conv.blur.kernel.copy_(asym_fir(4.0))
    assert dec._blur_factor() is None
